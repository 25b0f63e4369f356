"""Hand-made read batches for the seeding kernels (csrc/seed_kernels.hip against the reference's bwt_smem1 / bwt_sa): every structural limit of
the pack, forward, backward, filter, expand and locate kernels and of the fused form, each reached on purpose.  Plain numpy plus the oracle's rank
function, no tests, no GPU.

One genome of 160 kb is shared (world("main"): random bases with three planted structures, below); the capacity batches have a small one of their
own (world("small"): 8 kb with one A-run of 2 000 bases), so that their reads occur once or a thousand times and not 60 000 times.

A case is one batch: the ASCII bytes as the device gets them (`ascii`, with `shift` unused bytes in front: the tensor handed over is a view at that
byte offset of its allocation), offsets, lengths, min_seed_len, the genome, and `must`: name -> bool, what the case is about.  Every predicate is
evaluated when the case is built, on a restatement in Python of the split pipeline (restate(): the forward search's candidates with the iteration
that appends them, the chunked appends, the (read, ordinal) order, the backward walks in lockstep inside a wave, the filter's three ways to its
partner, expand and locate).  A generator that stops producing its edge fails the test that checks `must`.

Planted in the main genome (world("main").at):
  run     an A-run of 65 535 bases, the only homopolymer run longer than 18
  stair   a staircase: a 12-base context C, then U[:j] and a base that differs from U[j], for every j in 19..329 of a random 330-mer U, then one full
          C + U.  A read .. C U has a pass that starts inside C with a candidate at nearly every base of U: some 310 candidates of one pass
  mers    a 40-mer for each of 2, 4, 5, 63, 64, 65 and 129, planted that many times between A's (a read brings other flanks)
"""
from __future__ import annotations

import ctypes as C
import functools
import hashlib
import os
from types import SimpleNamespace

import numpy as np

MAX_K = 18
# csrc/seed_kernels.hip
CAND_CHUNK, PACK_READS_PER_BLOCK, LDS_MAX, SMALL, LOCATE_PER_WAVE, MAX_READ = 1024, 64, 65536, 4, 512, 65535
GENOME_LEN, RUN_AT, RUN_LEN, STAIR_AT, MERS_AT, PLAIN_AT = 160_000, 2_000, 65_535, 70_000, 130_000, 145_100
MER_COUNTS = (2, 4, 5, 63, 64, 65, 129)
PACK_COUNTS = (1, 63, 64, 65, 255, 256, 257)
PACK_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 992, 993)
SEED_KEYS = ("rbeg", "qbeg", "score", "n_ref_pos", "prefix")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seed_cases.npz")
M64 = (1 << 64) - 1

_NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _NT4[ord(_c)] = _NT4[ord(_c.lower())] = _i


def nt4(ascii_bytes):
    """the code of every letter (csrc/seed_kernels.hip: ascii_code): A C G T in either case, anything else 4"""
    return _NT4[np.asarray(ascii_bytes, np.uint8)]


def to_ascii(codes):
    return np.frombuffer(b"ACGTN", np.uint8)[np.asarray(codes, np.uint8)]


def revcomp(x):
    x = np.asarray(x, np.uint8)[::-1]
    return np.where(x < 4, 3 - x, 4).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the K-mer bitmap, restated
def kmer_k(seq_len: int) -> int:
    """the sizing rule: the smallest K with 4^K >= 8 seq_len, at most 18"""
    K = 1
    while K < MAX_K and 4 ** K < 8 * seq_len:
        K += 1
    return K


def text_of(g: np.ndarray) -> np.ndarray:
    return np.concatenate([g, 3 - g[::-1]]).astype(np.uint8)


def kmer_keys(t: np.ndarray, K: int) -> np.ndarray:
    """key of every length-K window of t: symbol j of the window at bits 2j+1:2j"""
    n = len(t) - K + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    key = np.zeros(n, np.uint64)
    for j in range(K):
        key |= t[j:j + n].astype(np.uint64) << np.uint64(2 * j)
    return key


def kmer_table(g: np.ndarray, K: int) -> np.ndarray:
    """bool [4^K]: does the K-mer occur in fwd . revcomp(fwd)"""
    tab = np.zeros(4 ** K, bool)
    tab[kmer_keys(text_of(g), K)] = True
    return tab


def window_alive(tab: np.ndarray, K: int, q: np.ndarray, e: int) -> bool:
    w = q[e - K:e]
    if e < K or (w > 3).any():
        return False
    return bool(tab[int(kmer_keys(w, K)[0])])


# ---------------------------------------------------------------------------------------------------------------- one read, restated
def smems_by_rule(orc, f, q: np.ndarray, min_seed_len: int, tab=None, K: int = 0, detail: dict | None = None):
    """One read through the split pipeline's decomposition, in plain Python over the oracle's rank function: forward candidates at
    every interval-size change, an independent backward walk for each, too-short results marked, contained results dropped by the
    next valid result of the read.  tab: candidates shorter than K whose window is dead are not generated at all.
    Returns ([(begin, end, k, s)], number of candidates, rank steps of the backward walks).
    detail: a dict that receives, in (ordinal) order, cands = [(x, end, k, s, pass, iteration of the forward kernel's loop that appends it)],
    res = [(begin, end, lo, s or 0)], sizes = [the interval size before the walk and after each of its steps], and every row pair the searches
    rank: fwd = [(k, l, s)] (rows l - 1 and l - 1 + s), bwd = [(lo, hi)] (rows lo - 1 and hi)."""
    occ = orc.lib.fmd_occ
    fp = C.byref(f)
    L2 = [int(f.L2[i]) for i in range(5)]
    primary, n = int(f.primary), len(q)
    use = tab is not None and min_seed_len >= K

    def occ4(k):
        return [int(occ(fp, k & M64, c)) for c in range(4)]
    cands, fwd, i, it, npass = [], [], 0, 0, 0
    while i < n:
        it += 1                                              # ST_START reads base i
        if q[i] > 3:
            i += 1
            continue
        x, b = i, int(q[i])
        k, s, l = L2[b] + 1, L2[b + 1] - L2[b], L2[3 - b] + 1
        i += 1
        if i == n:                                           # a pass that starts on the last base: appended by ST_START itself
            cands.append((x, i, k, s, npass, it))
            break
        while True:
            it += 1                                          # ST_EXT, or ST_TAIL behind the last base
            if i == n or q[i] > 3:
                cands.append((x, i, k, s, npass, it))
                break
            cb = 3 - int(q[i])
            tk, tl = occ4(l - 1), occ4(l - 1 + s)
            fwd.append((k, l, s))
            ns = [tl[c] - tk[c] for c in range(4)]
            nk = [0] * 4
            nk[3] = k + (1 if l <= primary <= l + s - 1 else 0)
            nk[2] = nk[3] + ns[3]; nk[1] = nk[2] + ns[2]; nk[0] = nk[1] + ns[1]
            if ns[cb] != s:
                cands.append((x, i, k, s, npass, it))
            if ns[cb] == 0:
                break                                    # the next pass starts at i
            k, l, s = nk[cb], L2[cb] + 1 + tk[cb], ns[cb]
            i += 1
        npass += 1
    cands = [c for c in cands if c[1] >= min_seed_len]
    if use:
        cands = [c for c in cands if c[1] - c[0] >= K or window_alive(tab, K, q, c[1])]
    res, steps, bwd, sizes = [], 0, [], []
    for x, e, k, s, _, _ in cands:
        lo, hi, beg, p = k, k + s - 1, x, x - 1
        sz = [s]
        while p >= 0 and q[p] < 4:
            b = int(q[p])
            steps += 1
            bwd.append((lo, hi))
            nl, nu = L2[b] + int(occ(fp, (lo - 1) & M64, b)) + 1, L2[b] + int(occ(fp, hi, b))
            if nl > nu:
                break
            lo, hi, beg, p = nl, nu, p, p - 1
            sz.append(hi - lo + 1)
        sizes.append(sz)
        res.append((beg, e, lo, hi - lo + 1 if e - beg >= min_seed_len else 0))
    out, nxt = [], None
    for beg, e, lo, s in reversed(res):                      # nxt: the next valid result behind this one
        if s == 0:
            continue
        if nxt is None or nxt[0] != beg:
            out.append((beg, e, lo, s))
        nxt = (beg, e, lo, s)
    out.reverse()
    if detail is not None:
        detail.update(cands=cands, res=res, sizes=sizes, fwd=fwd, bwd=bwd)
    return out, len(cands), steps


# ---------------------------------------------------------------------------------------------------------------- the genomes
def longest_runs(g):
    """(start, length) of every homopolymer run longer than 18"""
    cut = np.flatnonzero(np.diff(g.astype(np.int16)) != 0) + 1
    st = np.concatenate([[0], cut]); ln = np.diff(np.concatenate([st, [len(g)]]))
    return [(int(a), int(b)) for a, b in zip(st, ln) if b > 18]


MORE_WORLDS = {}


@functools.lru_cache(maxsize=None)
def world(which="main"):
    """genome, index, text, the oracle's handle on the index, and where the planted structures lie (at)"""
    import oracle_py
    from bwamem_hip import fmindex
    at = {}
    if which in MORE_WORLDS:                                   # (a table beside this one brings a genome of its own: tests/reseed_cases.py)
        g = MORE_WORLDS[which](at)
    elif which == "small":
        rng = np.random.default_rng(20262)
        g = rng.integers(0, 4, size=8_000).astype(np.uint8)
        g[3000:5000] = 0; g[2999] = 1; g[5000] = 2
        at["run"] = (3000, 2000)
    else:
        rng = np.random.default_rng(20263)
        g = rng.integers(0, 4, size=GENOME_LEN).astype(np.uint8)
        g[RUN_AT:RUN_AT + RUN_LEN] = 0; g[RUN_AT - 1] = 1; g[RUN_AT + RUN_LEN] = 2
        at["run"] = (RUN_AT, RUN_LEN)
        ctx, U = rng.integers(0, 4, size=12).astype(np.uint8), rng.integers(0, 4, size=330).astype(np.uint8)
        p = STAIR_AT
        for j in range(19, 330):
            piece = np.concatenate([ctx, U[:j], [(U[j] + 1 + j % 3) & 3]]).astype(np.uint8)
            g[p:p + len(piece)] = piece; p += len(piece)
        g[p:p + 342] = np.concatenate([ctx, U]); at["stair_full"] = p; p += 342
        assert p < MERS_AT
        at["stair"] = (STAIR_AT, p); at["ctx"], at["U"] = ctx, U
        p, mers = MERS_AT, {}
        for cnt in MER_COUNTS:
            m = rng.integers(0, 4, size=40).astype(np.uint8)
            m[0] = 1 + m[0] % 3; m[-1] = 1 + m[-1] % 3               # (no A at either end: the A's around a copy bound the match)
            mers[cnt] = m
            for _ in range(cnt):
                g[p:p + 45] = np.concatenate([[0], m, [0], 1 + rng.integers(0, 3, size=3)]); p += 45
        assert p < PLAIN_AT
        at["mers"] = mers
    assert longest_runs(g) == ([at["run"]] if "run" in at else []), longest_runs(g)
    idx = fmindex.build_fmd_index(g)
    orc = oracle_py.Oracle()
    f = orc.fmd(idx)
    # (sample 0 is reached through the row of suffix 0 alone, and only where that row is no sample itself)
    assert which != "main" or (int(idx.primary) % 16 and int(idx.primary) % 4), idx.primary
    g.setflags(write=False)
    return SimpleNamespace(name=which, g=g, idx=idx, text=text_of(g), orc=orc, f=f, at=at, digest=hashlib.sha1(g.tobytes()).hexdigest())


def sa_of(w, row):
    return int(w.orc.lib.fmd_sa(C.byref(w.f), int(row), None))


# ---------------------------------------------------------------------------------------------------------------- a batch, restated
_read_cache = {}


def _read_detail(w, q, msl):
    key = (w.name, q.tobytes(), msl)
    if key not in _read_cache:
        d = {}
        out, nc, steps = smems_by_rule(w.orc, w.f, q, msl, detail=d)
        d["out"], d["steps"] = out, steps
        _read_cache[key] = d
    return _read_cache[key]


def staging(c):
    """pack_reads_kernel's choice for every block of 64 reads: (in order, fits the LDS, aligned); it stages where all three hold"""
    max_len = int(c.lens.max(initial=0))
    n_grp = max(1, (max_len + 31) // 32)
    lds = PACK_READS_PER_BLOCK * n_grp * 32 + 64
    lds = lds if lds <= LDS_MAX else 0
    out = []
    for r0 in range(0, len(c.lens), PACK_READS_PER_BLOCK):
        r1 = min(r0 + PACK_READS_PER_BLOCK, len(c.lens)) - 1
        first, last = int(c.offs[r0]), int(c.offs[r1]) + int(c.lens[r1])
        out.append((last >= first, last >= first and (last - (first & ~3)) + 4 <= lds, c.shift % 4 == 0))
    return out


def slots_handed_out(cand_read, cand_iter):
    """cand_append, restated: every wave of 64 reads takes CAND_CHUNK slots at a time and leaves the rest of a chunk when a round does not fit.
    -> the counter's value behind the forward kernel (rank-walk form, no bitmap)"""
    total = 0
    wave = cand_read // 64
    for wv in np.unique(wave):
        rounds = np.bincount(cand_iter[wave == wv])
        cur = end = 0
        for n in rounds[rounds > 0].tolist():
            if cur + n > end:
                total += CAND_CHUNK; cur, end = 0, CAND_CHUNK
            cur += n
    return total


def restate(c):
    """the split pipeline on a whole case (default form: no text, no bitmap, one backward launch)"""
    w = world(c.genome)
    rd, xs, es, ks, ss, ps, its, begs, los, rs, nsteps, sizes = ([] for _ in range(12))
    smems, fwd, bwd, steps = [], [], [], 0
    for r in range(len(c.lens)):
        d = _read_detail(w, c.codes(r), c.msl)
        for (x, e, k, s, p, it), (beg, _, lo, s_out), sz in zip(d["cands"], d["res"], d["sizes"]):
            rd.append(r); xs.append(x); es.append(e); ks.append(k); ss.append(s); ps.append(p); its.append(it)
            begs.append(beg); los.append(lo); rs.append(s_out); sizes.append(sz)
        smems += [(r,) + t for t in d["out"]]
        fwd += d["fwd"]; bwd += d["bwd"]; steps += d["steps"]
    A = lambda v: np.array(v, np.int64)
    R = SimpleNamespace(read=A(rd), x=A(xs), e=A(es), k=A(ks), s=A(ss), pas=A(ps), it=A(its), beg=A(begs), lo=A(los), s_out=A(rs), sizes=sizes,
                        smems=smems, fwd=fwd, bwd=bwd, steps=steps, n_cands=len(rd), case=c)
    n = R.n_cands
    # the backward walks in lockstep: a segment is the run of one pass's candidates inside one wave; after every step a candidate whose size equals that of
    # the nearest longer one still walking stops and is marked dropped
    R.dropped = np.zeros(n, bool)
    t = 0
    while t < n:
        u = t + 1
        while u < n and u // 64 == t // 64 and R.read[u] == R.read[t] and R.x[u] == R.x[t]:
            u += 1
        x = int(R.x[t])
        if u - t > 1 and x > 0:
            lanes = list(range(t, u))
            act = {v: True for v in lanes}
            size = {v: sizes[v][0] for v in lanes}
            it = 0
            while any(act.values()):
                for v in lanes:
                    if act[v]:
                        if it + 1 < len(sizes[v]):
                            size[v] = sizes[v][it + 1]; act[v] = it + 1 < x
                        else:
                            act[v] = False
                now = [v for v in lanes if act[v]]
                for a, b in zip(now[:-1], now[1:]):
                    if size[a] == size[b]:
                        act[a] = False; R.dropped[a] = True
                it += 1
        t = u
    R.valid = (R.s_out > 0) & ~R.dropped
    # the filter: the partner of a valid result is the next valid one, whatever its read
    nxt = np.full(n + 1, n, np.int64)
    for t in range(n - 1, -1, -1):
        nxt[t] = t if R.valid[t] else nxt[t + 1]
    R.partner = nxt[1:]
    has = R.partner < n
    pp = np.minimum(R.partner, max(n - 1, 0))
    same = has & (R.read[pp] == R.read) & (R.beg[pp] == R.beg) if n else np.zeros(0, bool)
    R.kept = R.valid & ~same
    tt = np.arange(n)
    R.way = np.where(~has, 0, np.where(pp // 64 == tt // 64, 1, np.where(pp // 256 == tt // 256, 2, 3)))      # 1 ballot, 2 LDS, 3 the walk through global memory
    R.n_smems, R.n_seeds = int(R.kept.sum()), int(R.s_out[R.kept].sum())
    assert sorted(smems) == sorted(zip(R.read[R.kept].tolist(), R.beg[R.kept].tolist(), R.e[R.kept].tolist(), R.lo[R.kept].tolist(), R.s_out[R.kept].tolist()))
    R.slots = slots_handed_out(R.read, R.it) if n else 0
    rows = [v for k, l, s in fwd for v in (l - 1, l - 1 + s)] + [v for lo, hi in bwd for v in (lo - 1, hi)]
    R.rows = A(rows).reshape(-1, 2) if rows else np.zeros((0, 2), np.int64)
    return R


def walk_to_sample(w, row, intv):
    """locate_kernel's walk from a row: (the sampled row it ends on, steps)"""
    fp, steps = C.byref(w.f), 0
    while row % intv:
        row = int(w.orc.lib.fmd_inv_psi(fp, row)); steps += 1
    return row, steps


def reaches_sample0(R, intv):
    w = world(R.case.genome)
    return any(walk_to_sample(w, int(lo) + u, intv)[0] == 0 for lo, s in zip(R.lo[R.kept], R.s_out[R.kept]) for u in range(int(s)))


# ---------------------------------------------------------------------------------------------------------------- building cases
class Batch:
    """the reads of one case, in order; laid out back to back unless `layout` says otherwise"""

    def __init__(self, name, family, msl=19, genome="main", shift=0):
        self.name, self.family, self.msl, self.genome, self.shift = name, family, msl, genome, shift
        self.w = world(genome)
        self.rng = np.random.default_rng(int(hashlib.sha1(name.encode()).hexdigest()[:8], 16))
        self.reads = []

    def at(self, p, ln=150):
        return self.w.g[p:p + ln].copy()

    def plain(self, i, ln=150):
        """a read from the structure-free end of the genome"""
        return self.at(PLAIN_AT + (i * 197) % (GENOME_LEN - PLAIN_AT - ln - 10), ln)

    def rand(self, n):
        return self.rng.integers(0, 4, size=int(n)).astype(np.uint8)

    def add(self, codes=None, ascii_bytes=None):
        self.reads.append(np.asarray(to_ascii(codes) if ascii_bytes is None else np.frombuffer(bytes(ascii_bytes), np.uint8), np.uint8))
        return len(self.reads) - 1

    def case(self, must, layout="packed"):
        lens = np.array([len(r) for r in self.reads], np.uint32)
        n = len(lens)
        if layout == "packed":
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint32) if n else np.zeros(0, np.uint32)
            buf = np.concatenate(self.reads) if n and lens.sum() else np.zeros(0, np.uint8)
        elif layout == "descending":                               # the first read lies last in the buffer
            ends = np.cumsum(lens[::-1])[::-1]
            offs = (ends - lens).astype(np.uint32)
            buf = np.concatenate(self.reads[::-1])
        elif layout == "gaps":                                     # 3 unused bytes behind every read, 20 000 behind read 30
            offs, parts, o = np.zeros(n, np.uint32), [], 0
            for r, x in enumerate(self.reads):
                gap = 20_000 if r == 30 else 3
                offs[r] = o; parts += [x, np.full(gap, ord("#"), np.uint8)]; o += len(x) + gap
            buf = np.concatenate(parts)
        else:
            raise ValueError(layout)
        return make_case(self.name, self.family, buf, offs, lens, self.msl, self.genome, self.shift, must)


def make_case(name, family, buf, offs, lens, msl, genome, shift, must):
    c = SimpleNamespace(name=name, family=family, ascii=np.ascontiguousarray(buf, dtype=np.uint8), offs=np.ascontiguousarray(offs, dtype=np.uint32),
                        lens=np.ascontiguousarray(lens, dtype=np.uint32), msl=int(msl), genome=genome, shift=int(shift))
    assert len(c.offs) == len(c.lens) and (c.lens <= MAX_READ).all()
    assert all(int(o) + int(l) <= len(c.ascii) for o, l in zip(c.offs, c.lens)), name
    c.all_codes = nt4(c.ascii)
    c.codes = lambda r: c.all_codes[int(c.offs[r]):int(c.offs[r]) + int(c.lens[r])]
    h = hashlib.sha1()
    for part in (c.ascii.tobytes(), c.offs.tobytes(), c.lens.tobytes(), repr((c.msl, c.genome, c.shift, world(genome).digest)).encode()):
        h.update(part)
    c.digest = h.hexdigest()
    c.R = restate(c)
    c.stage = staging(c)
    c.must = {what: bool(f(c, c.R)) for what, f in must.items()}
    assert c.must, name
    return c


def sub(r, *pos):
    for p in pos:
        if 0 <= p < len(r):
            r[p] = (r[p] + 1 + p % 3) & 3
    return r


def staged_all(c, R):
    return all(all(b) for b in c.stage)


def finds_every_plain_read(c, R):
    return R.n_smems >= int((c.lens >= 40).sum()) > 0


# ---- packing
def case_pack_count(n):
    B = Batch("pack_count_%d" % n, "packing")
    for i in range(n):
        B.add(sub(B.plain(i, 40), 25) if i & 1 else B.plain(i, 40))
    return B.case({"%d reads, every block staged" % n: lambda c, R: len(c.lens) == n and staged_all(c, R) and len(c.stage) == (n + 63) // 64,
                   "every read is found": finds_every_plain_read})


def _length_reads(B, lengths, mixed):
    for i, ln in enumerate(lengths):
        B.add(sub(B.plain(3 * i, ln), ln // 3, (2 * ln) // 3) if ln >= 60 else B.plain(3 * i, ln))
        if mixed:
            for k in range(7):
                B.add(sub(B.plain(100 + 8 * i + k), 70))


def case_pack_lengths(top, mixed):
    lengths = tuple(l for l in PACK_LENGTHS if l <= top)
    B = Batch("pack_len_%d%s" % (top, "_mixed" if mixed else ""), "packing")
    _length_reads(B, lengths, mixed)
    fits = top <= 992
    return B.case({"the lengths": lambda c, R: set(lengths) <= set(c.lens.tolist()) and int(c.lens.max()) == top,
                   "64 reads of %d bases %s the LDS" % (top, "fit" if fits else "do not fit"): lambda c, R: all(b == (True, fits, True) for b in c.stage),
                   "more than one block": lambda c, R: not mixed or len(c.stage) > 1,
                   "the long reads are found": lambda c, R: R.n_smems >= 2})


def case_pack_last_empty():
    B = Batch("pack_last_empty", "packing")
    for i in range(67):
        B.add(B.plain(i, 40) if i != 63 else np.zeros(0, np.uint8))
    return B.case({"the first block's last read is empty": lambda c, R: c.lens[63] == 0 and len(c.stage) == 2 and staged_all(c, R), "every read is found": finds_every_plain_read})


def case_pack_letters():
    B = Batch("pack_letters", "packing")
    iupac = b"RYKMSWBDHVNnryU-.*"
    for i in range(66):
        a = bytearray(to_ascii(B.plain(i)).tobytes())
        if i % 3 == 0:
            a = bytearray(bytes(a).lower())
        elif i % 3 == 1:
            a = bytearray(bytes(ch | 0x20 if k & 1 else ch for k, ch in enumerate(a)))
        if i % 4 == 1:
            a[40 + i] = iupac[(i // 4) % len(iupac)]
        if i % 4 == 2:
            a[30 + i] = (0, 255, 1, 0x41 | 0x80, 0x61 | 0x80, ord("@"), 0x7F, ord("a") ^ 0x40)[(i // 4) % 8]    # bytes one bit away from a base's letter among them
        B.add(ascii_bytes=bytes(a))
    return B.case({"lower case, IUPAC letters and other bytes": lambda c, R: any(97 <= v <= 122 for v in c.ascii.tolist()) and (c.all_codes == 4).sum() >= 30
                   and len(set(c.ascii[c.all_codes == 4].tolist())) >= 20,
                   "every read is found": finds_every_plain_read})


def case_pack_layout(layout):
    B = Batch("pack_" + layout, "packing")
    for i in range(70):
        B.add(sub(B.plain(i), 50 + i))
    want = {"gaps": [(True, False, True), (True, True, True)], "descending": [(False, False, True)] * 2}[layout]
    return B.case({"staging: " + repr(want): lambda c, R: c.stage == want, "every read is found": finds_every_plain_read}, layout=layout)


def case_pack_shared():
    """reads that share bytes: read i begins 10 bytes behind read i - 1"""
    B = Batch("pack_shared", "packing")
    n = 70
    stretch = sub(B.at(PLAIN_AT + 500, 150 + 10 * (n - 1)), 333, 555)
    offs = (10 * np.arange(n)).astype(np.uint32)
    return make_case(B.name, B.family, to_ascii(stretch), offs, np.full(n, 150, np.uint32), 19, "main", 0,
                     {"two reads share bytes, the blocks are staged": lambda c, R: int(c.offs[1]) < int(c.offs[0]) + int(c.lens[0]) and staged_all(c, R),
                      "every read is found": finds_every_plain_read})


def case_pack_view(shift):
    B = Batch("pack_view_%d" % shift, "packing", shift=shift)
    for i in range(70):
        B.add(sub(B.plain(i + shift), 60 + i))
    return B.case({"the ASCII pointer is %d bytes off a dword: nothing is staged" % shift: lambda c, R: c.stage == [(True, True, False)] * 2, "every read is found": finds_every_plain_read})


# ---- nothing found
def case_none(kind):
    B = Batch("none_" + kind, "nothing")
    for i in range(65):
        B.add({"empty": lambda: np.zeros(0, np.uint8), "N": lambda: np.full(30 + i, 4, np.uint8), "short": lambda: B.plain(i, i % 19),
               "nowhere": lambda: B.rand(40 + i)}[kind]())
    must = {"no seeds": lambda c, R: R.n_smems == 0 and R.n_seeds == 0}
    if kind == "nowhere":       # (a read from nowhere still has candidates: every one of them ends too short)
        must["candidates, all too short"] = lambda c, R: R.n_cands > 64 and not R.valid.any()
    else:
        must["no candidates"] = lambda c, R: R.n_cands == 0
    return B.case(must)


# ---- passes
def stair_read(B, lead):
    w = B.w
    return np.concatenate([lead, w.at["ctx"], w.at["U"]]).astype(np.uint8)


def big_pass(R):
    """(first, last) candidate of the largest pass with x > 0"""
    best = (0, 0)
    t = 0
    while t < R.n_cands:
        u = t
        while u < R.n_cands and R.read[u] == R.read[t] and R.pas[u] == R.pas[t]:
            u += 1
        if R.x[t] > 0 and u - t > best[1] - best[0]:
            best = (t, u)
        t = u
    return best


def case_stairs():
    """the staircase read behind 30..33 genomic bases from elsewhere (the lanes of the forward wave append out of step), behind an N and at the read's start (walks of
    length 0); plain reads in front move the big passes across wave and block boundaries"""
    B = Batch("stairs", "passes")
    for i in range(3):
        B.add(sub(B.plain(i), 75))
    for k in range(4):
        B.add(stair_read(B, B.plain(40 + k, 30 + k)))
    B.add(stair_read(B, np.concatenate([B.plain(50, 20), [4]])))
    B.add(stair_read(B, np.zeros(0, np.uint8)))

    def straddles(c, R):
        a, b = big_pass(R)
        return a // 64 != (b - 1) // 64 and a // 256 != (b - 1) // 256

    def zero_walks(c, R):
        big = [(int(R.x[t]), int(R.read[t])) for t in range(R.n_cands) if len(R.sizes[t]) == 1]
        return sum(1 for x, r in big if x == 0) > 256 and sum(1 for x, r in big if x > 0 and c.codes(r)[x - 1] == 4) > 256
    return B.case({
        "a pass with x > 0 has more than 256 candidates": lambda c, R: big_pass(R)[1] - big_pass(R)[0] > 256,
        "it straddles a wave and a block in (read, ordinal) order": straddles,
        "a contained candidate sits in another wave than its longer mate": lambda c, R: bool((R.valid & ~R.kept & (R.way >= 2)).any()),
        "a contained result's longer mate lies in the next block": lambda c, R: bool((R.valid & ~R.kept & (R.way == 3)).any()),
        "the four shifted reads append their last candidates in four different iterations": lambda c, R: len({int(R.it[R.read == r][-1]) for r in (3, 4, 5, 6)}) == 4,
        "big passes at x = 0 and behind an N: walks of length 0": zero_walks,
        "candidates that would be long enough are dropped in lockstep": lambda c, R: int((R.dropped & (R.s_out > 0)).sum()) > 256,
        "an SMEM covers the staircase in every read": lambda c, R: all(any(s[0] == r and s[2] == c.lens[r] and s[2] - s[1] >= 342 for s in R.smems) for r in range(3, 9))})


def case_lockstep():
    """reads with substitutions: the candidates of a pass walk back into unique sequence, their sizes meet and the shorter ones stop"""
    B = Batch("lockstep", "passes")
    for i in range(40):
        r = sub(B.plain(i), 40 + i, 90 + i)
        B.add(revcomp(r) if i & 1 else r)
    return B.case({"candidates are dropped in lockstep": lambda c, R: int(R.dropped.sum()) >= 40,
                   "passes cross wave boundaries": lambda c, R: any(R.read[t] == R.read[t - 1] and R.pas[t] == R.pas[t - 1] for t in range(64, R.n_cands, 64))})


# ---- filter
def case_filter():
    """a read whose first SMEM is followed by more than 512 results that end too short (700 bases from nowhere) and then by a second SMEM: the partner of the
    first one lies blocks away"""
    B = Batch("filter_far", "filter")
    for i in range(3):
        B.add(np.concatenate([B.plain(10 * i, 40), B.rand(700), B.plain(10 * i + 5, 40)]))
        B.add(sub(B.plain(20 + i), 33, 99))
    kept_way = lambda R, wy: bool((R.kept & (R.way == wy)).any())

    def far(c, R):
        t = np.flatnonzero(R.kept & (R.way == 3))
        return any(R.partner[u] - u > 256 and R.read[R.partner[u]] == R.read[u] for u in t)
    return B.case({"a kept result's partner lies in its wave": lambda c, R: kept_way(R, 1), "... in a later wave of its block": lambda c, R: kept_way(R, 2),
                   "... in a later block of the same read, invalid results between them": far,
                   "a kept result is the batch's last valid one": lambda c, R: bool((R.kept & (R.way == 0)).any())})


# ---- rank rows
def case_rank_rows():
    B = Batch("rank_rows", "ranks")
    w = B.w
    prim = int(w.idx.primary)
    n2 = len(w.text)
    for row in (prim - 1, prim, prim + 1):
        p = sa_of(w, row)
        body = w.text[p:p + 40]
        B.add(np.concatenate([[(int(w.text[p - 1]) + 1) & 3 if p else 1], body]))
    for i in range(100):
        B.add(sub(B.plain(i), 30 + i % 90, 100 + i % 40))
    rows_hit = lambda R, v: bool((R.rows == v).any())
    return B.case({"a forward step's interval holds the primary row": lambda c, R: any(l <= prim <= l + s - 1 for k, l, s in R.fwd),
                   "rows primary - 1, primary, primary + 1 and seq_len are ranked": lambda c, R: all(rows_hit(R, v) for v in (prim - 1, prim, prim + 1, n2)),
                   "a pair lies in one block": lambda c, R: bool(((R.rows[:, 0] >> 6) == (R.rows[:, 1] >> 6)).any()),
                   "pairs end on offsets 0 and 63 of a block": lambda c, R: bool(((R.rows & 63) == 0).any() and ((R.rows & 63) == 63).any())})


# ---- expand and locate
def mer_read(B, cnt):
    return np.concatenate([1 + B.rand(25) % 3, [1], B.w.at["mers"][cnt], [2], 1 + B.rand(25) % 3]).astype(np.uint8)


def case_occ_counts():
    B = Batch("occ_counts", "expand")
    B.add(B.plain(7, 60))
    for cnt in MER_COUNTS:
        B.add(mer_read(B, cnt))
    return B.case({"SMEMs of 1, 2, 4, 5, 63, 64, 65 and 129 occurrences": lambda c, R: {1, *MER_COUNTS} <= {s[4] for s in R.smems},
                   "both sides of the lane / wave switch of expand_kernel": lambda c, R: {SMALL, SMALL + 1} <= set(R.s_out[R.kept].tolist())})


def case_occ_total(total):
    B = Batch("occ_total_%d" % total, "expand")
    for cnt in (129, 129, 129, 64) + (5,) * 12:
        B.add(mer_read(B, cnt))
    assert total - 511 in (0, 1, 2) and LOCATE_PER_WAVE == 512         # one wave of locate_kernel short of one occurrence, full, and a second wave for one
    if total - 511 == 1:
        B.add(B.plain(9, 60))
    if total - 511 == 2:
        B.add(mer_read(B, 2))
    return B.case({"%d occurrences in all" % total: lambda c, R: R.n_seeds == total})


def case_text_edges():
    B = Batch("text_edges", "expand")
    w = B.w
    n = len(w.g)
    for p in range(17):
        B.add(w.text[p:p + 40])
    B.add(w.text[n - 40:n]); B.add(w.text[n - 20:n + 20]); B.add(w.text[n - 1:n + 39]); B.add(w.text[2 * n - 40:2 * n])
    B.add(revcomp(w.text[0:40]))
    return B.case({"a located row reaches sample 0 at a sampling interval of 16": lambda c, R: reaches_sample0(R, 16),
                   "... and of 4": lambda c, R: reaches_sample0(R, 4),
                   "text positions 0..16 are found": lambda c, R: all(any(s[0] == r and s[1] == 0 and s[2] == 40 for s in R.smems) for r in range(17)),
                   "every read is found": lambda c, R: len({s[0] for s in R.smems}) == len(c.lens)})


# ---- long
def case_long_polya():
    B = Batch("long_polyA", "long")
    B.add(sub(B.plain(1), 70)); B.add(np.zeros(MAX_READ, np.uint8)); B.add(B.plain(2, 40)); B.add(sub(B.plain(3), 20, 120))
    return B.case({"65 517 candidates in one pass": lambda c, R: int((R.read == 1).sum()) == MAX_READ - 19 + 1 == 65517 and len(set(R.pas[R.read == 1].tolist())) == 1,
                   "the fused form's scratch depth max_len - min_seed_len + 1 is met exactly": lambda c, R: int((R.read == 1).sum()) == int(c.lens.max()) - c.msl + 1,
                   "one SMEM, one occurrence": lambda c, R: [(s[1], s[2], s[4]) for s in R.smems if s[0] == 1] == [(0, MAX_READ, 1)],
                   "ends up to 65 535": lambda c, R: int(R.e.max()) == MAX_READ})


def case_capacity(length):
    """57 poly-A reads and 7 empty ones: one forward wave whose rounds are 57 appends each, so that every chunk of 1024 slots is left with 55 unused"""
    B = Batch("capacity_%d" % length, "long", genome="small")
    for i in range(64):
        B.add(np.zeros(length if i < 57 else 0, np.uint8))
    bases = 57 * length
    over = length == 2000             # (1 000 bases are over as well: 982 rounds take 58 chunks, 59 392 slots against 59 176)

    def slots(c, R):
        return R.n_cands == 57 * (length - 18) and (R.slots > R.n_cands + (64 // 64 + 1) * (CAND_CHUNK + 64)) and (R.slots > bases + 2 * 1088) == over
    return B.case({"slots handed out exceed candidates + (64/64 + 1) 1088%s" % (", and one per base + 2 176" if over else ", not one per base + 2 176"): slots,
                   "57 SMEMs": lambda c, R: R.n_smems == 57 and R.n_seeds == 57 * (2000 - length + 1)})


def case_long_2000():
    B = Batch("long_2000", "long")
    r = sub(B.at(PLAIN_AT + 3000, 2000), *range(60, 2000, 97))
    B.add(r); B.add(revcomp(r)); B.add(B.plain(4, 40))
    return B.case({"a 2 000-base read in pieces": lambda c, R: sum(1 for s in R.smems if s[0] == 0) >= 15 and int(c.lens.max()) == 2000,
                   "unique intervals grow forward over many bases": lambda c, R: sum(1 for k, l, s in R.fwd if s == 1) > 1000})


# ---- options
def case_mixed(msl):
    B = Batch("mixed_msl%d" % msl, "options", msl=msl)
    for i in range(30):
        r = sub(B.plain(2 * i), 20 + i, 75, 130 - i)
        if i % 5 == 0:
            r[60] = 4
        B.add(revcomp(r) if i % 3 == 0 else r)
    for ln in (11, 12, 13, 18, 19, 20, 24, 25, 26):
        B.add(B.plain(77 + ln, ln))
    B.add(B.rand(100))
    must = {"min_seed_len %d: seeds" % msl: lambda c, R: c.msl == msl and R.n_smems >= 30,
            "interval sizes stay below 2^32, the batch's occurrences below 20 000": lambda c, R: int(R.s.max()) < 1 << 32 and R.n_seeds < 20_000}
    if msl == 1:
        must["one-base candidates"] = lambda c, R: bool((R.e - R.x == 1).any())
    return B.case(must)


BUILDERS = {}
for _n in PACK_COUNTS:
    BUILDERS["pack_count_%d" % _n] = functools.partial(case_pack_count, _n)
for _top, _mixed in ((992, False), (993, False), (992, True), (993, True)):
    BUILDERS["pack_len_%d%s" % (_top, "_mixed" if _mixed else "")] = functools.partial(case_pack_lengths, _top, _mixed)
BUILDERS.update(pack_last_empty=case_pack_last_empty, pack_letters=case_pack_letters, pack_gaps=functools.partial(case_pack_layout, "gaps"),
                pack_descending=functools.partial(case_pack_layout, "descending"), pack_shared=case_pack_shared)
for _s in (1, 2, 3):
    BUILDERS["pack_view_%d" % _s] = functools.partial(case_pack_view, _s)
for _k in ("empty", "N", "short", "nowhere"):
    BUILDERS["none_" + _k] = functools.partial(case_none, _k)
BUILDERS.update(stairs=case_stairs, lockstep=case_lockstep, filter_far=case_filter, rank_rows=case_rank_rows, occ_counts=case_occ_counts)
for _t in (511, 512, 513):
    BUILDERS["occ_total_%d" % _t] = functools.partial(case_occ_total, _t)
BUILDERS.update(text_edges=case_text_edges, long_polyA=case_long_polya, capacity_500=functools.partial(case_capacity, 500),
                capacity_2000=functools.partial(case_capacity, 2000), long_2000=case_long_2000)
for _m in (1, 12, 19, 25):
    BUILDERS["mixed_msl%d" % _m] = functools.partial(case_mixed, _m)
NAMES = tuple(BUILDERS)
FAMILIES = ("packing", "nothing", "passes", "filter", "ranks", "expand", "long", "options")


@functools.lru_cache(maxsize=None)
def get(name):
    c = BUILDERS[name]()
    assert c.name == name
    return c


def all_cases():
    return {n: get(n) for n in NAMES}


# ---------------------------------------------------------------------------------------------------------------- the fixture
def reference_seeds(ref, bwts, c):
    """the compiled reference on a case: the columns common.assert_seeds_equal compares, and the number of SMEMs"""
    if c.genome not in bwts:
        bwts[c.genome] = ref.bwt_from_index(world(c.genome).idx)
    got = ref.seed_reads(bwts[c.genome], c.all_codes if len(c.all_codes) else np.zeros(1, np.uint8), c.offs.astype(np.uint64), c.lens, min_seed_len=c.msl)
    out = {k: got[k] for k in SEED_KEYS}
    out["n_smems"] = np.int64(len(got["smem_k"]))
    return out


def make_fixture(path=FIXTURE):
    """tests/golden/seed_cases.npz from the reference's library (oracle/_ref/libref.so, where it can be built)"""
    import oracle_py
    oracle_py.build(ref=True)
    ref, bwts, z = oracle_py.Ref(), {}, {}
    for name, c in all_cases().items():
        for k, v in reference_seeds(ref, bwts, c).items():
            z[name + "." + k] = v
        z[name + ".digest"] = np.array(c.digest)
    np.savez_compressed(path, **z)
    return path


def load_fixture(path=FIXTURE):
    """name -> the reference's columns.  A table edited without regenerating the fixture is refused."""
    z = np.load(path)
    out = {}
    for name in NAMES:
        c = get(name)
        assert name + ".digest" in z.files and str(z[name + ".digest"]) == c.digest, \
            "tests/seed_cases.py changed (%s): run seed_cases.make_fixture() where the reference's library can be built" % name
        out[name] = {k: z[name + "." + k] for k in SEED_KEYS}
        out[name]["n_smems"] = int(z[name + ".n_smems"])
        for v in out[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    assert {f.split(".")[0] for f in z.files} == set(NAMES)
    return out


if __name__ == "__main__":
    print(make_fixture())
