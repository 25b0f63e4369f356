"""Hand-made region sets for the region tail (csrc/regs_kernels.hip against the host form csrc/regs_post.cpp and the CPU build of
csrc/regs_core.h): every size class of the device form at its limits, ties of every sort key, a collision of the tie-break hash's short
key, deep dedup windows, the patch test's alignment in every band class, the marking and the selection at their thresholds, contig and
ALT tables.  Plain numpy, no tests, no GPU.

A region is the 8-int record the tail takes: [0] unused, [1] score, [2] qb, [3] qe, [4,5] rb, [6,7] re.  The genome is 64 kb of random
bases (L_PAC = 65536 = FIN_NLOG, so one region can cover 65535 or 65536 reference bases); a forward hit at P is rb = P, re = P + len,
a reverse hit covering forward [Q, Q + len) is rb = 2 L_PAC - (Q + len), re = 2 L_PAC - Q.  Every record is legal input (check_legal):
0 <= qb < qe <= read length, 0 <= rb < re <= 2 L_PAC, no region bridges L_PAC, and 0 <= score <= a * max(qe - qb, re - rb) -- the
MAPQ formula squares the identity 1 - (l a - score) / (a + b) / l, which leaves the range of an int for scores far beyond the length.

A case is one batch: reads, regions, options, tables and `must`, what the case is about: name -> True (a predicate on the input,
restated here in Python and evaluated when the case is built) or name -> function(result) judged from the host form's output
(result.per_read[r] = the [m, 16] records of read r).  A generator that stops producing its edge fails the test that checks `must`.

Sizes: every family that can runs at SIZES regions per read, both sides of every edge of the device form (FIN_NL = 8: lane kernel / wave
kernel; 32, 128, 256: the wave classes; FIN_NMAX = 512: LDS / HBM; 1024 = FIN_STAGE: one / two staged blocks of keys; 2049: three)."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

L_PAC = 65536
SIZES = (0, 1, 2, 8, 9, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2049)
FIN_NL, CLASS_CAPS, FIN_NMAX, FIN_STAGE, FIN_DPCAP, FIN_NLOG, FIN_CTG_LDS = 8, (32, 128, 256, 512), 512, 1024, 1024, 65536, 512
M64 = (1 << 64) - 1
# defaults of mem_opt_init (bmh_chain_opt_default / bmh_post_opt_default / ExtParams.default) the predicates below restate
DEF = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, w=100, min_seed_len=19, max_chain_gap=10000, mask_level=0.5, drop_ratio=0.5,
           T=30, mask_level_redun=0.95, mapQ_coef_len=50.0, mapQ_coef_fac=3)
# arguments whose hash64 values agree in their top 32 bits (found by a search of 2^25 arguments)
COLLIDE = ((6466637, 6466639), (31188963, 31188982))


def fin_class(n: int) -> int:
    """the wave class of a read of n regions (csrc/regs_kernels.hip: fin_class)"""
    return sum(n > c for c in CLASS_CAPS)


def hash64(key: int) -> int:
    """hash_64 of mem_mark_primary_se (csrc/regs_core.h: hash64)"""
    key &= M64
    key = (key + (~(key << 32) & M64)) & M64; key ^= key >> 22
    key = (key + (~(key << 13) & M64)) & M64; key ^= key >> 8
    key = (key + (key << 3)) & M64; key ^= key >> 15
    key = (key + (~(key << 27) & M64)) & M64; key ^= key >> 31
    return key


def pack_pac(g):
    pad = (-len(g)) % 4
    codes = np.concatenate([g, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    pac = ((codes[:, 0] << 6) | (codes[:, 1] << 4) | (codes[:, 2] << 2) | codes[:, 3]).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([pac, np.zeros(8, np.uint8)]))


@functools.lru_cache(maxsize=1)
def genome():
    g = np.random.default_rng(20260).integers(0, 4, size=L_PAC).astype(np.uint8)
    return g, pack_pac(g)


def revcomp(x):
    x = np.asarray(x, np.uint8)[::-1]
    return np.where(x < 4, 3 - x, 4).astype(np.uint8)


def rec(score, qb, qe, rb, re):
    return (0, int(score), int(qb), int(qe), int(rb) & 0xFFFFFFFF, int(rb) >> 32, int(re) & 0xFFFFFFFF, int(re) >> 32)


def to_rev(r):
    """the same hit seen from the other strand of a read of length r[-1]: (score, qb, qe, rb, re, L) -> the record on the reverse strand"""
    score, qb, qe, rb, re, L = r
    return (score, L - qe, L - qb, 2 * L_PAC - re, 2 * L_PAC - rb)


class Batch:
    """reads with their regions, in read order"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.reads, self.recs, self.rpr, self.frac, self.tags = [], [], [], [], []

    def add(self, bases, recs, frac=0.0, tag=""):
        """recs: (score, qb, qe, rb, re) in any order -> the read's index"""
        self.reads.append(np.ascontiguousarray(bases, dtype=np.uint8))
        self.recs += [rec(*r) for r in recs]
        self.rpr.append(len(recs)); self.frac.append(frac); self.tags.append(tag)
        return len(self.reads) - 1

    def random_read(self, L):
        return self.rng.integers(0, 4, size=L).astype(np.uint8)

    def case(self, name, must, co=None, ep=None, po=None, contigs=None, is_alt=None, device_error=None, core_error=0, families=(), reverse=False):
        order = list(range(len(self.reads)))
        if reverse:
            order = order[::-1]
        starts = np.concatenate([[0], np.cumsum(self.rpr)]).astype(np.int64)
        allr = np.array(self.recs, dtype=np.int64).reshape(-1, 8)
        regs = np.concatenate([allr[starts[r]:starts[r + 1]] for r in order] + [np.zeros((0, 8), np.int64)])
        g, pac = genome()
        c = SimpleNamespace(name=name, genome=g, pac=pac, reads=[self.reads[r] for r in order],
                            regs=np.ascontiguousarray(regs.astype(np.uint32).view(np.int32) if regs.size else np.zeros((0, 8), np.int32)),
                            rpr=np.array([self.rpr[r] for r in order], np.uint32), frac_rep=np.array([self.frac[r] for r in order], np.float32),
                            tags=[self.tags[r] for r in order], co=dict(co or {}), ep=dict(ep or {}), po=dict(po or {}), contigs=contigs,
                            is_alt=None if is_alt is None else np.ascontiguousarray(is_alt, dtype=np.uint8), must=dict(must),
                            device_error=device_error, core_error=core_error, families=tuple(families))
        c.po.setdefault("id0", 1234567)
        check_legal(c)
        return c


def fields(c):
    """the regions of a case as int64 columns: score, qb, qe, rb, re and the read of every region"""
    r = c.regs.astype(np.int64)
    u = lambda lo, hi: (r[:, lo] & 0xFFFFFFFF) | (r[:, hi] << 32)
    return r[:, 1], r[:, 2], r[:, 3], u(4, 5), u(6, 7), np.repeat(np.arange(len(c.rpr)), c.rpr.astype(np.int64))


def check_legal(c):
    score, qb, qe, rb, re, rd = fields(c)
    lens = np.array([len(x) for x in c.reads], np.int64)
    a = c.ep.get("a", DEF["a"])
    assert len(c.regs) == int(c.rpr.sum()) and len(c.reads) == len(c.rpr)
    assert (0 <= qb).all() and (qb < qe).all() and (qe <= lens[rd]).all(), c.name
    assert (0 <= rb).all() and (rb < re).all() and (re <= 2 * L_PAC).all(), c.name
    assert not ((rb < L_PAC) & (re > L_PAC)).any(), c.name
    assert (score >= 0).all() and (score <= a * np.maximum(qe - qb, re - rb)).all(), c.name
    assert len(c.regs) < 60_000 and (c.rpr <= 2100).all(), c.name


def read_slices(c):
    s = np.concatenate([[0], np.cumsum(c.rpr.astype(np.int64))])
    return [slice(int(s[r]), int(s[r + 1])) for r in range(len(c.rpr))]


# ---------------------------------------------------------------------------------------------------------------- predicates, restated
def rid_of(c, rb, re):
    """bns_pos2rid of a region's forward position (csrc/regs_core.h: init_one)"""
    pos = np.where(rb < L_PAC, rb, 2 * L_PAC - 1 - (re - 1))
    if not c.contigs or len(c.contigs) <= 1:
        return np.zeros(len(rb), np.int32)
    off = np.concatenate([[0], np.cumsum([x[1] for x in c.contigs])[:-1]])
    return (np.searchsorted(off, pos, side="right") - 1).astype(np.int32)


def patch_pre(opt, a, b):
    """the tests of mem_patch_reg before its alignment on regions a = (score, qb, qe, rb, re, w), b likewise (a.rb <= b.rb): None, or the band"""
    f32 = np.float32
    if a[3] < L_PAC and b[3] >= L_PAC:
        return None
    if a[1] >= b[1] or a[2] >= b[2] or a[4] >= b[4]:
        return None
    w = abs((a[4] - b[3]) - (a[2] - b[1]))
    r = abs((a[4] - b[3]) / (b[4] - a[3]) - (a[2] - b[1]) / (b[2] - a[1]))
    if a[4] < b[3] or a[2] < b[1]:
        if w > opt["w"] << 1 or r >= float(f32(0.05)):
            return None
    elif w > opt["w"] << 2 or r >= float(f32(0.05) * f32(2)):
        return None
    return min(w + a[5] + b[5], opt["w"] << 2)


def gen_plan(opt, w_, l_query, rb, re):
    """what bwa_gen_cigar2 does (csrc/regs_core.h: gen_plan): (plan, band, columns per lane of the wave form or 0 = lane 0 alone)"""
    rlen = re - rb
    if l_query == rlen and w_ == 0:
        return 1, 0, 0
    mi = int((((l_query + 1) >> 1) * opt["a"] - opt["o_ins"]) / opt["e_ins"] + 1.)
    md = int((((l_query + 1) >> 1) * opt["a"] - opt["o_del"]) / opt["e_del"] + 1.)
    mg = max(mi, md, 1)
    diff = abs(rlen - l_query)
    w = max(min((mg + diff + 1) >> 1, w_), diff + 3)
    if 2 * w + 1 > 512:
        return 2, w, 0
    widest = max(min(i + w + 1, l_query) - max(i - w, 0) for i in range(rlen))
    return 2, w, (widest + 63) >> 6


def dedup_scan(c, r, opt):
    """mem_sort_dedup_patch's scan on read r of a case whose regions have distinct `re` and never reach the patch test (asserted): what the wave form's
    64-lane steps must reproduce.  -> survivors, deepest window, deaths [(step, lane)] of region i against predecessor j, dead predecessors passed over"""
    score, qb, qe, rb, re, _ = (x[read_slices(c)[r]] if i < 5 else None for i, x in enumerate(fields(c)))
    assert len(set(re.tolist())) == len(re)
    o = np.argsort(re, kind="stable")
    score, qb, qe, rb, re = (x[o].tolist() for x in (score, qb, qe, rb, re))
    n, gap, redun = len(re), opt["max_chain_gap"], np.float32(opt["mask_level_redun"])
    dead = [False] * n
    deepest, deaths, passed = 0, [], 0
    for i in range(1, n):
        if not rb[i] < re[i - 1] + gap:
            continue
        j = i - 1
        while j >= 0 and rb[i] < re[j] + gap:
            deepest = max(deepest, i - j)
            if dead[j]:
                passed += 1; j -= 1; continue
            pr = re[j] - rb[i]
            pq = qe[j] - qb[i] if qb[j] < qb[i] else qe[i] - qb[j]
            mr = min(re[j] - rb[j], re[i] - rb[i]); mq = min(qe[j] - qb[j], qe[i] - qb[i])
            if np.float32(pr) > redun * np.float32(mr) and np.float32(pq) > redun * np.float32(mq):
                if score[i] < score[j]:
                    dead[i] = True; deaths.append(((i - 1 - j) // 64, (i - 1 - j) % 64)); break
                dead[j] = True
            else:
                assert not rb[j] < rb[i], "the restated scan does not run the patch test"
            j -= 1
    return n - sum(dead), deepest, deaths, passed


# ---------------------------------------------------------------------------------------------------------------- pieces of reads
def slots(rng, n, length=20):
    """n reference intervals of `length` bases in distinct 32-base slots over both strands (a slot never bridges L_PAC), in random order"""
    k = rng.permutation(2 * L_PAC // 32)[:n].astype(np.int64)
    rb = k * 32 + rng.integers(0, 32 - length + 1, size=n)
    return rb, rb + length


def scattered_read(B, n, same_score=0):
    """n regions far apart on the reference (nothing to dedup at max_chain_gap = 0), distinct scores (or one score for all): every key of the three sorts
    is unique but for the equal scores, which the hash then orders alone"""
    rng = B.rng
    L = n + 150
    rb, re = slots(rng, n)
    sc = np.full(n, same_score) if same_score else rng.permutation(n) + 20
    qb = rng.integers(0, 60, size=n)
    qe = qb + sc + rng.integers(0, 60, size=n)
    return B.random_read(L), list(zip(sc, qb, np.minimum(qe, L), rb, re))


def filler(B, n, L, base=L_PAC + 20000, score=20):
    """n regions that do nothing to one another: on the reverse strand, 32 bases apart, query starts falling while the reference rises (never colinear: the
    patch test refuses them before its alignment), query intervals of 20 bases"""
    i = np.arange(n)
    rb = base + 32 * i
    qb = (n - 1 - i) * (L - 20) // n                              # (never rising: a.qb >= b.qb refuses)
    return list(zip(np.full(n, score), qb, qb + 20, rb, rb + 20))


def cut_read(B, p0, pieces, flank=0):
    """a read cut from the genome at p0: pieces = [(length, gap)], `length` bases copied, then gap > 0: that many reference bases skipped (a deletion),
    gap < 0: that many random bases inserted, then the next piece.  -> bases, [(qb, qe, rb, re)] of the pieces on the forward strand"""
    g, _ = genome()
    out, segs, q, p = [], [], 0, p0
    for ln, gap in pieces:
        out.append(g[p:p + ln]); segs.append((q, q + ln, p, p + ln)); q += ln; p += ln
        if gap > 0:
            p += gap
        elif gap < 0:
            out.append((g[p - 1:p - 1 - gap] + 1 + B.rng.integers(0, 3, size=-gap).astype(np.uint8)) & 3); q += -gap       # (never the base the reference has next to it)
    return np.concatenate(out).astype(np.uint8), segs


def patch_read(B, p0, pieces, rev=False, mism=0, a=1, keep=None):
    """cut_read with one region per piece (score = a * length: plausible for an exact piece) on the forward or the reverse strand; mism: so many bases
    of the read next to every junction are changed (the alignment across the junction then scores less than the pieces promise)"""
    bases, segs = cut_read(B, p0, pieces)
    L = len(bases)
    for s in segs[:-1]:
        for k in range(mism):
            bases[s[1] - 1 - 2 * k] = (bases[s[1] - 1 - 2 * k] + 1) & 3
    recs = [(a * (s[1] - s[0]), s[0], s[1], s[2], s[3]) for k, s in enumerate(segs) if keep is None or k in keep]
    if rev:
        bases = revcomp(bases); recs = [to_rev(r + (L,)) for r in recs]
    return bases, recs


def plans_of(c, r, opt):
    """(plan, band, columns per lane) of the patch test between consecutive regions of read r, taken by `re`"""
    score, qb, qe, rb, re, _ = (x[read_slices(c)[r]] if i < 5 else None for i, x in enumerate(fields(c)))
    o = np.argsort(re, kind="stable")
    out = []
    for x, y in zip(o[:-1], o[1:]):
        a = (score[x], qb[x], qe[x], rb[x], re[x], opt["w"]); b = (score[y], qb[y], qe[y], rb[y], re[y], opt["w"])
        w = patch_pre(opt, [int(v) for v in a], [int(v) for v in b])
        out.append(None if w is None else gen_plan(opt, w, int(qe[y] - qb[x]), int(rb[x]), int(re[y])))
    return out


def _opt(**over):
    o = dict(DEF); o.update(over); return o


def n_out(r):
    return lambda res: len(res.per_read[r])


# ---------------------------------------------------------------------------------------------------------------- the families
def case_scattered(sizes=SIZES, name="scattered", reverse=False):
    B = Batch(1)
    uniq = True
    for n in sizes:
        b, recs = scattered_read(B, n)
        B.add(b, recs, tag="n%d" % n)
        uniq = uniq and len({x[0] for x in recs}) == n and len({x[4] for x in recs}) == n
    must = {"every sort key is unique": uniq, "a read at every size": sorted(B.rpr) == sorted(sizes),
            "nothing is removed": lambda res: [len(x) for x in res.per_read] == list(res.case.rpr)}
    return B.case(name, must, co=dict(max_chain_gap=0), families=("scattered",), reverse=reverse)


def case_ties(same=False):
    """equal `re` in groups, exact duplicates, one score for all regions of a read.  same: mask_level_redun = 1 -- two regions with one (score, rb, qb) are
    then not redundant for the scan (the overlap equals the shorter length, never exceeds it) and reach the second sort as a tie, where dedup_same drops one"""
    B = Batch(2)
    rng = B.rng
    want = []
    for n in SIZES:
        if n < 2:
            B.add(B.random_read(150), scattered_read(B, n)[1]); want.append(n); continue
        kind = len(B.reads) % 3
        L = n + 150
        if kind == 0 and not same:                                 # groups of four regions that end at one position, query intervals apart
            rb, re = slots(rng, (n + 3) // 4, length=32)
            recs = [(10 + (7 * i) % 11, 25 * (i % 4), 25 * (i % 4) + 24, re[i // 4] - 8 - 6 * (i % 4), re[i // 4]) for i in range(n)]
        elif kind == 1 or same:                                    # every region up to three times: once more as it is, once more with another end
            rb, re = slots(rng, (n + 2) // 3)
            sc = rng.integers(8, 20, size=len(rb))
            recs = []
            for i in range(n):
                k, v = divmod(i, 3)
                recs.append((sc[k], 40 + k % 50, 40 + k % 50 + 20 - (v == 2), rb[k], re[k] - (v == 2)))
        else:                                                      # one score: the marking order is the hash order
            recs = scattered_read(B, n, same_score=20)[1]
        B.add(B.random_read(L), recs)
        want.append(len({(x[0], x[3], x[1]) for x in recs}))
    score, qb, qe, rb, re, rd = None, None, None, None, None, None
    must = {"regions with equal re": True, "exact duplicates": True}
    c = B.case("ties_same" if same else "ties", must, co=dict(max_chain_gap=0), po=dict(mask_level_redun=1.0) if same else {}, families=("ties",))
    score, qb, qe, rb, re, rd = fields(c)
    sl = read_slices(c)
    c.must["regions with equal re"] = any(len(set(re[s].tolist())) < (s.stop - s.start) for s in sl)
    c.must["exact duplicates"] = any(len({(a_, b_, c_) for a_, b_, c_ in zip(score[s].tolist(), rb[s].tolist(), qb[s].tolist())}) < (s.stop - s.start) for s in sl)
    if not same:
        c.must["a read with one score and more than 64 regions"] = any(s.stop - s.start > 64 and len(set(score[s].tolist())) == 1 for s in sl)
    if same:                                                       # only dedup_same removes anything: one region per (score, rb, qb) is left
        c.must["dedup_same leaves one region per (score, rb, qb)"] = lambda res: [len(x) for x in res.per_read] == want and sum(want) < len(res.case.regs)
    return c


def case_wide():
    """scores of 16384 and more (the sort's 128-bit keys) beside a read that stops at 16383 (the 64-bit keys); a = 2 as on a 16 kb read; regions of score 0"""
    B = Batch(3)
    rng = B.rng
    tops = {}
    for n, top in ((2, 16384), (9, 16383), (9, 16384), (33, 16383), (33, 16384), (129, 40000), (513, 16384), (513, 16383), (1025, 17000)):
        rb, re = slots(rng, n)
        sc = top - np.arange(n) * (1 if top < 40000 else 150)
        sc[-1] = 0                                                  # the last one scores nothing
        o = rng.permutation(n)
        qb = rng.integers(0, 100, size=n)
        lq = max(8192, (top + 1) // 2)                                # (a = 2: a score of 16384 takes 8192 bases)
        recs = [(sc[i], qb[i], qb[i] + lq + 20 * (i % 60), rb[i], re[i]) for i in o]
        tops[B.add(B.random_read(lq + 1400), recs)] = top
    # a primary whose only overlapping regions score 0 (its sub stays 0), then one that scores; and a read of nothing but zeros
    rb, re = slots(rng, 6)
    B.add(B.random_read(200), [(60, 0, 60, rb[0], re[0]), (0, 0, 50, rb[1], re[1]), (0, 5, 60, rb[2], re[2]), (40, 100, 160, rb[3], re[3]), (0, 100, 150, rb[4], re[4])])
    zr = B.add(B.random_read(200), [(0, 0, 50, rb[0], re[0]), (0, 0, 50, rb[1], re[1]), (0, 100, 150, rb[5], re[5])])
    must = {"a read whose top score is 16383 and one with 16384": {16383, 16384} <= set(tops.values()),
            "regions of score 0 come through": lambda res: len(res.per_read[zr]) == 3 and (res.per_read[zr][:, 1] == 0).all(),
            "sub skips the zero scores": lambda res: res.per_read[zr - 1][0, 10] == 0 and res.per_read[zr - 1][0, 1] == 60}
    return B.case("wide", must, co=dict(max_chain_gap=0, a=2), ep=dict(a=2), families=("wide",))


def case_collision(pair, alt):
    """Two records of one read whose tie-break hashes agree in their top 32 bits, with one score (and one ALT flag): the short key of the marking sort
    (score | top 32 bits of the hash; 31 bits in the order that puts the primary assembly first) cannot tell them apart and the second, full-key round has to."""
    x, y = COLLIDE[pair]
    B = Batch(4 + pair)
    n, i1, r_col = max(12, y - x + 6), 3, 2
    for _ in range(r_col):
        B.add(*scattered_read(B, 9))
    contigs, is_alt = None, None
    if alt:                                                        # two sequences, the second an ALT one: the reverse strand of the first half ... is sequence 1's
        contigs, is_alt = [("c0", L_PAC // 2), ("c1_alt", L_PAC // 2)], np.array([0, 1], np.uint8)
    # regions of one score in the first sequence (forward strand), list position = rank by rb; with a table a few ALT hits of a lower score make the second sort run
    rb = np.arange(n) * 64 + 1000
    recs = [(50, 3 * i, 3 * i + 50, rb[i], rb[i] + 50) for i in range(n)]
    if alt:
        recs += [(40, 3 * i, 3 * i + 50, L_PAC // 2 + 64 * i, L_PAC // 2 + 64 * i + 50) for i in range(4)]
    o = B.rng.permutation(len(recs))
    B.add(B.random_read(3 * n + 60), [recs[i] for i in o])
    B.add(*scattered_read(B, 33))
    id0 = x - r_col - i1
    hx, hy = hash64(id0 + r_col + i1), hash64(id0 + r_col + i1 + (y - x))
    must = {"the two hashes share their top 32 bits and differ": hx >> 32 == hy >> 32 and hx != hy, "the read has 12 regions or more": n >= 12,
            "both records are in the list with one score": lambda res: len(res.per_read[r_col]) == len(recs) and (res.per_read[r_col][:n, 1] == 50).all()}
    return B.case("collision%d%s" % (pair, "_alt" if alt else ""), must, co=dict(max_chain_gap=0), po=dict(id0=id0), contigs=contigs, is_alt=is_alt, families=("collision",))


def case_tandem():
    """regions of one strand inside max_chain_gap of one another.  `nested` reads: every region contains the ones before it on the reference (the patch test is
    never reached: a predecessor never starts to the left), the query intervals fall into clusters -- a region is redundant with the predecessors of its cluster,
    dies against a better one deep inside its window or outlives them all and scans to the window's end; `free` reads: random overlapping regions, some colinear
    (the patch test runs its alignment on whatever bases the random read has)"""
    B = Batch(6)
    rng = B.rng
    nested = []
    for n in SIZES:
        for rev in (0, 1):
            if n > 600 and rev:
                continue
            base = 3000 + L_PAC * rev
            i = np.arange(n)
            ncl = max(3, n // 12)
            cl = rng.integers(0, ncl, size=n)
            L = 20 * ncl + 40
            qb = 20 * cl + rng.integers(0, 2, size=n)
            sc = rng.integers(10, 19, size=n)
            recs = list(zip(sc, qb, qb + 18, base - 50 - i, base + 1 + i))
            o = rng.permutation(n)
            nested.append(B.add(B.random_read(L), [recs[k] for k in o], tag="nested"))
    # redundancy is not transitive: region 12 covers the query intervals of regions 5 (better: region 12 dies there, on lane 6 of its first step) and 0
    # (weaker, not redundant with region 5, so still there; lane 11 of the same step would empty it had region 12 lived) -- region 0 must come through
    base = 40000
    recs = [(12, 300 + 20 * k, 318 + 20 * k, base - 50 - k, base + 1 + k) for k in range(40)]
    recs[0] = (10, 0, 20, base - 50, base + 1); recs[5] = (18, 100, 120, base - 55, base + 6); recs[12] = (14, 0, 120, base - 62, base + 13)
    hazard = B.add(B.random_read(1200), [recs[k] for k in rng.permutation(40)], tag="hazard")
    for n in (2, 8, 9, 33, 65, 129, 257):
        L = 400
        i = np.arange(n)
        rb = 30000 + 7 * i + rng.integers(0, 5, size=n)
        ln = rng.integers(80, 120, size=n)
        qb = rng.integers(0, L - 130, size=n)
        qe = qb + rng.integers(80, 120, size=n)
        B.add(B.random_read(L), list(zip(rng.integers(40, 80, size=n), qb, qe, rb, rb + ln)), tag="free")
    c = B.case("tandem", {}, families=("tandem",))
    scans = {r: dedup_scan(c, r, DEF) for r in nested if 64 < c.rpr[r] <= 513}
    deaths = [d for s in scans.values() for d in s[2]]
    c.must.update({
        "windows reach beyond 64 and beyond 128 predecessors": max(s[1] for s in scans.values()) > 128 and any(64 < s[1] <= 128 for s in scans.values()),
        "a region dies inside a 64-lane step, in the first step and in later ones": any(st == 0 and 0 < ln < 63 for st, ln in deaths) and any(st >= 2 and 0 < ln < 63 for st, ln in deaths),
        "a region dies on the first and on the last lane of a step": any(ln == 0 for _, ln in deaths) and any(ln == 63 for _, ln in deaths),
        "emptied predecessors lie inside windows": all(s[3] > 0 for s in scans.values()),
        "the restated scan leaves what the host form leaves": lambda res: all(len(res.per_read[r]) == s[0] for r, s in scans.items()),
        "a region dies in the middle of a step whose later lanes hold a weaker redundant predecessor": lambda res: len(res.per_read[hazard]) == 39 and
        dedup_scan(c, hazard, DEF)[2] == [(0, 6)] and sorted(res.per_read[hazard][:, 1].tolist())[:1] == [10] and 14 not in res.per_read[hazard][:, 1],
        "free reads lose regions": lambda res: any(t == "free" and len(x) < k for t, x, k in zip(res.case.tags, res.per_read, res.case.rpr)),
    })
    return c


def _patch_batch(B, w, a=1):
    """the patch reads for band option w: (what, read, regions in, regions expected out or None)"""
    rng = B.rng
    info = []
    P = lambda: int(rng.integers(1000, 20000))

    def add(what, bases, recs, want, extra=0):
        if extra:
            recs = recs + filler(B, extra, len(bases))
        o = rng.permutation(len(recs))
        info.append((what, B.add(bases, [recs[i] for i in o], tag=what), len(recs), want))

    if w == 0:       # equal gaps on both sides (a stretch of mismatches between the pieces): the ungapped plan
        for rev in (False, True):
            bases, segs = cut_read(B, P(), [(150, 0)])
            bases[72] = (bases[72] + 1) & 3; bases[75] = (bases[75] + 2) & 3
            recs = [(70, 0, 70, segs[0][2], segs[0][2] + 70), (72, 78, 150, segs[0][2] + 78, segs[0][3])]
            if rev:
                bases = revcomp(bases); recs = [to_rev(r + (150,)) for r in recs]
            add("ungapped", bases, recs, 1)
        return info
    d = {5: 4, 20: 5, 100: 6}[w]
    for rev in (False, True):
        add("deletion", *patch_read(B, P(), [(130, d), (140, 0)], rev=rev, a=a), 1)
        add("insertion", *patch_read(B, P(), [(140, -d), (130, 0)], rev=rev, a=a), 1)
        add("rejected", *patch_read(B, P(), [(60, d), (60, 0)], rev=rev, mism=3, a=a), 2)
        add("three", *patch_read(B, P(), [(130, d), (120, d - 1), (140, 0)], rev=rev, a=a), 1)
    if w == 5:
        # an insertion of 12 bases, 60 bases on, a deletion of 14: the band (12) holds the path that takes the insertion first and not the one that takes the
        # deletion first -- walking both sequences backwards (a window on the reverse strand) is not the same alignment as walking them forwards
        for rev in (False, True):
            add("asym", *patch_read(B, P(), [(400, -12), (60, 14), (400, 0)], rev=rev, a=a, keep=(0, 2)), None)
    if w == 100:
        for n in (9, 33, 129, 257, 513, 1025):                     # the alignment in every wave class: a pair among n regions
            add("class", *patch_read(B, P(), [(300, 9), (300, 0)], rev=False, a=a), n - 1, extra=n - 2)
        for L1, dd in ((300, 20), (450, 30)):                      # wider bands: more columns per lane
            add("wide band", *patch_read(B, P(), [(L1, dd), (L1, 0)], rev=bool(L1 & 64), a=a), 1)
        # lane 0 alone (2 w + 1 > 512): a band of 256 takes a query side beyond 1000 bases and regions that bring bands of their own -- the third piece
        # meets a region that was merged with a band of 220
        for rev in (False, True):
            add("lane0", *patch_read(B, P(), [(340, 20), (340, 12), (330, 0)], rev=rev, a=a), 1)
        for side in (1021, 1022):                                  # the longest query sides the device's alignment scratch holds
            add("side%d" % side, *patch_read(B, P(), [(500, 10), (side - 500, 0)], a=a), 1)
        # a forward and a reverse region next to each other around L_PAC: the patch test refuses them by their strands
        bases = B.random_read(150)
        add("strands", bases, [(60, 0, 60, L_PAC - 100, L_PAC - 40), (60, 70, 130, L_PAC + 20, L_PAC + 80)], 2)
    return info


def case_patch(w):
    B = Batch(10 + w)
    info = _patch_batch(B, w)
    c = B.case("patch_w%d" % w, {}, co=dict(w=w), families=("patch",))
    opt = _opt(w=w)
    plans = {r: plans_of(c, r, opt) for what, r, n, _ in info if n <= 3}
    kinds = {what for what, *_ in info}
    cols = sorted({p[2] for ps in plans.values() for p in ps if p and p[0] == 2})
    for what, r, n, _ in info:                                     # the second merge of a lane0 read, with the band its first merge leaves
        if what == "lane0":
            score, qb, qe, rb, re, _ = (x[read_slices(c)[r]] if i < 5 else None for i, x in enumerate(fields(c)))
            o = np.argsort(re)
            A, Bm, Cc = ([int(x[k]) for x in (score, qb, qe, rb, re)] + [w] for k in o)
            w1 = patch_pre(opt, A, Bm)
            merged = [0, A[1], Bm[2], A[3], Bm[4], w1]
            plans[r] = plans[r][:1] + [gen_plan(opt, patch_pre(opt, merged, Cc), Cc[2] - merged[1], merged[3], Cc[4])]
    cols = sorted({p[2] for ps in plans.values() for p in ps if p and p[0] == 2})
    c.must["every read does what it was built for"] = lambda res: all(want is None or len(res.per_read[r]) == want for _, r, _, want in info)
    c.must["the patch test reaches its alignment in every small read"] = all(ps[0] is not None for r, ps in plans.items() if c.tags[r] != "strands")
    if w == 0:
        c.must["the ungapped plan"] = all(p[0] == 1 for ps in plans.values() for p in ps)
    if w == 5:
        c.must["one column per lane"] = cols == [1]
        asym = [r for what, r, _, _ in info if what == "asym"]
        # (walked from the insertion's end the path stays 12 columns off the diagonal, inside the band of 12; from the other end it would start 14 off)
        c.must["both strands find the path the band holds from one end only"] = lambda res: all(
            len(res.per_read[r]) == 1 and res.per_read[r][0, 1] == 860 - (6 + 12) - (6 + 14) and res.per_read[r][0, 9] == 12 for r in asym)
    if w == 20:
        c.must["two to eight columns per lane"] = any(2 <= x <= 8 for x in cols) and 0 not in cols
    if w == 100:
        c.must["several columns per lane and lane 0 alone"] = 0 in cols and len([x for x in cols if 2 <= x <= 8]) >= 3
        c.must["merged regions carry the band they were merged with"] = lambda res: any(t == "three" and x[0, 9] != w for t, x in zip(res.case.tags, res.per_read))
        c.must["reads of every wave class and of the lane kernel's size"] = {fin_class(n) for _, _, n, _ in info} == {0, 1, 2, 3, 4} and any(n <= FIN_NL for _, _, n, _ in info)
        c.must["strands refuse"] = "strands" in kinds
    c.must["accepted and rejected merges, both strands"] = w == 0 or {"deletion", "insertion", "rejected", "three"} <= kinds
    return c


def case_patch_toolong():
    """a query side of 1023 bases: one more than the device's alignment scratch holds (FIN_DPCAP - 2); the host form answers"""
    B = Batch(30)
    B.add(*scattered_read(B, 9))
    bases, recs = patch_read(B, 5000, [(500, 10), (523, 0)])
    r = B.add(bases, recs)
    B.add(*scattered_read(B, 40))
    return B.case("patch_side1023", {"the host form merges the pair": lambda res: len(res.per_read[r]) == 1 and res.per_read[r][0, 3] - res.per_read[r][0, 2] == 1023},
                  families=("patch",), device_error="patch alignment beyond the kernel's capacity")


def case_scoring():
    """the patch reads under another scoring (a = 2: scores and penalties doubled but the mismatch, which then decides the marking's window)"""
    B = Batch(31)
    info = _patch_batch(B, 100, a=2)
    over = dict(a=2, b=9, o_del=12, e_del=2, o_ins=12, e_ins=2)
    c = B.case("patch_scoring", {}, co=dict(over), ep=dict(over), po=dict(T=60), families=("patch",))
    c.must["merges happen"] = lambda res: sum(len(res.per_read[r]) == 1 for what, r, n, _ in info if n <= 3) >= 8
    return c


def case_mark():
    B = Batch(40)
    rng = B.rng
    must = {}
    tmp = 7                                                        # max(a + b, o_del + e_del, o_ins + e_ins) of the defaults
    # a pair whose query overlap is one short of, exactly, and one beyond mask_level of the shorter region (100 bases, mask_level 0.5)
    for ov in (49, 50, 51):
        rb, re = slots(rng, 2)
        r = B.add(B.random_read(260), [(100, 0, 100, rb[0], re[0]), (90, 100 - ov, 200 - ov, rb[1], re[1])])
        must["overlap %d of 100" % ov] = (lambda r, ov: lambda res: (res.per_read[r][1, 12] >= 0) == (ov >= 50))(r, ov)
    # sub_n: a runner-up at the score window's edge and one beyond it
    for diff in (tmp, tmp + 1):
        rb, re = slots(rng, 2)
        r = B.add(B.random_read(260), [(100, 0, 100, rb[0], re[0]), (100 - diff, 0, 100, rb[1], re[1])])
        must["sub_n at a score difference of %d" % diff] = (lambda r, diff: lambda res: res.per_read[r][0, 11] == (diff <= tmp) and res.per_read[r][0, 10] == 100 - diff)(r, diff)
    # n disjoint primaries: query intervals of two bases
    for n in (64, 65, 512, 513):
        rb, re = slots(rng, n)
        o = rng.permutation(n)
        r = B.add(B.random_read(2 * n + 10), [(10 + (i * 7) % 11, 2 * i, 2 * i + 2, rb[i], re[i]) for i in o])
        must["%d primaries" % n] = (lambda r, n: lambda res: len(res.per_read[r]) == n and (res.per_read[r][:, 12] == -1).all())(r, n)
    # clusters of three regions: the best of a cluster becomes a primary inside a 64-step and claims the other two, which may lie in the same step
    late = []
    for n, L in ((60, 400), (200, 1400), (520, 3600)):
        rb, re = slots(rng, n)
        o = rng.permutation(n)
        late.append(B.add(B.random_read(L), [(20 - (i % 3) * (1 + i % 2) - (i // 3) % 2, 20 * (i // 3), 20 * (i // 3) + 20, rb[i], re[i]) for i in o]))

    def same_step(res):
        ok = []
        for r in late:
            sec = res.per_read[r][:, 12]
            i = np.nonzero(sec >= 1)[0]
            ok.append(bool(((sec[i] - 1) // 64 == (i - 1) // 64).any()) and bool(((sec[i] - 1) // 64 < (i - 1) // 64).any() or len(sec) <= 64))
        return all(ok)
    must["primaries found inside a step claim regions of that step"] = same_step
    return B.case("mark", must, co=dict(max_chain_gap=0), families=("mark",))


def case_mark_ab():
    """sub_n where a + b is the window: b = 9 (a + b = 10 beyond o + e = 7)"""
    B = Batch(41)
    must = {}
    for diff in (10, 11):
        rb, re = slots(B.rng, 2)
        r = B.add(B.random_read(260), [(100, 0, 100, rb[0], re[0]), (100 - diff, 0, 100, rb[1], re[1])])
        must["sub_n at a score difference of %d" % diff] = (lambda r, diff: lambda res: res.per_read[r][0, 11] == (diff <= 10))(r, diff)
    B.add(*scattered_read(B, 33))
    return B.case("mark_ab", must, co=dict(max_chain_gap=0, b=9), ep=dict(b=9), families=("mark",))


def case_emit(flag_all=0, no_multi=0):
    B = Batch(50)
    rng = B.rng
    must = {}
    T = DEF["T"]
    for sc in (T, T - 1):
        rb, re = slots(rng, 1, length=32)
        r = B.add(B.random_read(100), [(sc, 0, 40, rb[0], re[0])])
        must["score %d" % sc] = (lambda r, sc: lambda res: (res.per_read[r][0, 15] & 1) == (sc >= T))(r, sc)
    for sc in (50, 49):                                            # drop_ratio 0.5 of a primary of 100
        rb, re = slots(rng, 2)
        r = B.add(B.random_read(200), [(100, 0, 100, rb[0], re[0]), (sc, 0, 100, rb[1], re[1])])
        must["a secondary of %d under a primary of 100" % sc] = (lambda r, sc: lambda res: (res.per_read[r][1, 15] & 1) == (flag_all and sc >= 50) and res.per_read[r][1, 14] == 0x100)(r, sc)
    # a primary with a close runner-up (low MAPQ), then a unique hit elsewhere in the read: supplementary, its MAPQ capped by the first record's
    rb, re = slots(rng, 3)
    r = B.add(B.random_read(300), [(100, 0, 100, rb[0], re[0]), (97, 0, 100, rb[1], re[1]), (90, 150, 250, rb[2], re[2])])
    must["the supplementary record's MAPQ is capped"] = lambda res: res.per_read[r][2, 14] == (0x10000 if no_multi else 0x800) and 0 < res.per_read[r][2, 13] == res.per_read[r][0, 13] < 30
    for fr in (0.0, 0.37, 1.0):
        rb, re = slots(rng, 1, length=32)
        q = B.add(B.random_read(100), [(80, 0, 80, rb[0], re[0])], frac=fr)
        must["frac_rep %g" % fr] = (lambda q, fr: lambda res: res.per_read[q][0, 13] == int(60 * (1. - float(np.float32(fr))) + .499))(q, fr)
    for l in (49, 50, 51):                                         # mapQ_coef_len = 50
        rb, re = slots(rng, 1, length=20)
        B.add(B.random_read(100), [(l - 6, 0, l, rb[0], re[0])], tag="len%d" % l)
    for n in (9, 70, 300):                                         # ordinary reads around them
        B.add(*scattered_read(B, n))
    r65535 = B.add(B.random_read(200), [(150, 0, 150, 0, 65535), (60, 20, 100, L_PAC + 40, L_PAC + 120)])
    must["a region of 65535 reference bases"] = lambda res: len(res.per_read[r65535]) == 2 and res.per_read[r65535][0, 15] & 1
    name = "emit" + ("_all" if flag_all else "") + ("_nomulti" if no_multi else "")
    return B.case(name, must, co=dict(max_chain_gap=0), po=dict(flag_all=flag_all, no_multi=no_multi), families=("emit",))


def case_emit_65536():
    """a region of 65536 reference bases: beyond the device's logarithm table (and the CPU core's: the same limit); the host form answers"""
    B = Batch(51)
    B.add(*scattered_read(B, 9))
    r = B.add(B.random_read(200), [(150, 0, 150, 0, 65536), (60, 20, 100, L_PAC + 40, L_PAC + 120)])
    B.add(*scattered_read(B, 40))
    return B.case("emit_65536", {"the host form answers": lambda res: len(res.per_read[r]) == 2 and res.per_read[r][0, 15] & 1}, co=dict(max_chain_gap=0),
                  families=("emit",), device_error="logarithm table", core_error=-2)


def contig_table(n):
    """L_PAC bases cut into n sequences"""
    if n == 1:
        return [("c0", L_PAC)]
    base = L_PAC // n
    lens = [base] * (n - 1) + [L_PAC - base * (n - 1)]
    return [("c%d" % i, x) for i, x in enumerate(lens)]


def case_contigs(n_ctg, alt=False, flag_all=0):
    """regions in the first, the last and random sequences of a table of n_ctg, both strands, default max_chain_gap: a window ends where the sequence
    changes.  alt: every third sequence (and the last) is an ALT one; reads without ALT hits, with nothing else, and mixed"""
    B = Batch(60 + n_ctg + alt)
    rng = B.rng
    contigs = contig_table(n_ctg)
    off = np.concatenate([[0], np.cumsum([x[1] for x in contigs])]).astype(np.int64)
    is_alt = None
    if alt:
        is_alt = np.zeros(n_ctg, np.uint8); is_alt[2::3] = 1; is_alt[-1] = 1
    kinds = []
    for n in SIZES:
        if n > 600 and n_ctg in (2, 513):
            continue
        L = 400
        which = len(B.reads) % 3                                   # ALT tables: 0 = the primary assembly only, 1 = ALT sequences only, 2 = mixed
        pool = np.arange(n_ctg) if not alt or which == 2 else np.nonzero(is_alt == (which == 1))[0]
        ctg = pool[rng.integers(0, len(pool), size=n)]
        if n >= 2:
            ctg[0], ctg[1] = pool[0], pool[-1]
        ln = 24
        room = (off[ctg + 1] - off[ctg]) - ln
        p = off[ctg] + (rng.integers(0, 1 << 30, size=n) % np.maximum(room, 1))
        rev = rng.integers(0, 2, size=n).astype(bool)
        if n >= 2 and (not alt or which == 2):
            rev[0], rev[1], p[0], p[1] = False, True, 0, L_PAC - ln   # the first bases of the first sequence, the last of the last one on the reverse strand
        rb = np.where(rev, 2 * L_PAC - (p + ln), p)
        qb = rng.integers(0, L - 60, size=n)
        sc = rng.integers(10, 24, size=n)
        kinds.append(which)
        B.add(B.random_read(L), list(zip(sc, qb, qb + rng.integers(24, 60, size=n), rb, rb + ln)), tag="k%d" % which)
    co = {}
    must = {"the table has %d sequences" % n_ctg: len(contigs) == n_ctg and sum(x[1] for x in contigs) == L_PAC}
    if alt:
        must["ALT hits, shadowed hits and ALT hits with a parent"] = lambda res: (res.out[:, 15] & 2).any() and (res.out[:, 15] >> 2 > 0).any() and (res.out[:, 12] == 0x7FFFFFFF).any()
        must["reads without ALT hits, with nothing else, and mixed"] = lambda res: all(
            any(t == "k%d" % k and len(x) > 1 and {0: not (x[:, 15] & 2).any(), 1: (x[:, 15] & 2).all(), 2: 0 < ((x[:, 15] & 2) > 0).sum() < len(x)}[k]
                for t, x in zip(res.case.tags, res.per_read)) for k in (0, 1, 2))
    c = B.case("contigs%d%s%s" % (n_ctg, "_alt" if alt else "", "_all" if flag_all else ""), must, co=co, po=dict(flag_all=flag_all), contigs=contigs, is_alt=is_alt,
               families=("contigs",) + (("alt",) if alt else ()))
    score, qb, qe, rb, re, _ = fields(c)
    rid = rid_of(c, rb, re)
    c.must["regions in the first and the last sequence, both strands"] = bool(((rid == 0) & (rb < L_PAC)).any() and ((rid == n_ctg - 1) & (rb >= L_PAC)).any() and
                                                                                ((rid == 0) & (rb >= L_PAC)).any() and ((rid == n_ctg - 1) & (rb < L_PAC)).any()) or n_ctg == 1
    return c


def case_late_first():
    """ALT mode: 70 hits of the primary assembly below T, then ALT hits that are reported -- the first reported record lies in the second 64-step"""
    B = Batch(70)
    contigs, is_alt = [("c0", L_PAC // 2), ("c1_alt", L_PAC // 2)], np.array([0, 1], np.uint8)
    recs = [(20, 6 * i, 6 * i + 6, 200 + 40 * i, 230 + 40 * i) for i in range(70)]
    recs += [(60 - i, 500 + 70 * i, 560 + 70 * i, L_PAC // 2 + 300 + 100 * i, L_PAC // 2 + 360 + 100 * i) for i in range(3)]
    o = B.rng.permutation(len(recs))
    B.add(*scattered_read(B, 9))
    r = B.add(B.random_read(800), [recs[i] for i in o])
    must = {"the first reported record is record 70": lambda res: (np.nonzero(res.per_read[r][:, 15] & 1)[0] == np.array([70, 71, 72])).all()
            and res.per_read[r][71, 14] == 0x800}
    return B.case("late_first", must, co=dict(max_chain_gap=0), contigs=contigs, is_alt=is_alt, families=("emit", "alt"))


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = [case_scattered(), case_scattered(name="scattered_reversed", reverse=True),
          case_scattered(sizes=tuple(n for n in SIZES if not 128 < n <= 256), name="scattered_class2_empty"),      # one wave class holds no read
          case_ties(False), case_ties(True), case_wide()]
    cs += [case_collision(p, a) for p in (0, 1) for a in (False, True)]
    cs += [case_tandem()] + [case_patch(w) for w in (0, 5, 20, 100)] + [case_patch_toolong(), case_scoring()]
    cs += [case_mark(), case_mark_ab(), case_emit(), case_emit(flag_all=1), case_emit(no_multi=1), case_emit_65536()]
    cs += [case_contigs(n) for n in (1, 2, 512, 513)] + [case_contigs(n, alt=True, flag_all=f) for n, f in ((2, 0), (512, 0), (513, 1))] + [case_late_first()]
    assert len({c.name for c in cs}) == len(cs)
    return {c.name: c for c in cs}


NAMES = ("scattered", "scattered_reversed", "scattered_class2_empty", "ties", "ties_same", "wide", "collision0", "collision0_alt", "collision1", "collision1_alt",
         "tandem", "patch_w0", "patch_w5", "patch_w20", "patch_w100", "patch_side1023", "patch_scoring", "mark", "mark_ab", "emit", "emit_all", "emit_nomulti",
         "emit_65536", "contigs1", "contigs2", "contigs512", "contigs513", "contigs2_alt", "contigs512_alt", "contigs513_alt_all", "late_first")


def get(name):
    return all_cases()[name]
