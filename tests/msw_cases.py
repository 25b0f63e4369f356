"""Hand-made jobs for the mate rescue's local alignment (csrc/pair_kernels.hip against the host walk csrc/local_sw.cpp and the reference's
ksw_align2): every length class of the four kernel forms at its limits, waves of mixed lengths and widths, batches that do not fill a block,
targets around the staging buffer's refills, the edges of the 2-bit text, the letters a read can hold, insertions whose F crosses from one
SSE lane into the next, the second-best bookkeeping at its boundaries, the tie rules, the KSW_XSUBO threshold, six scorings and the byte
pass's overflow.  Plain numpy, no tests, no GPU.

A case is one batch: its own small genome (codes 0..3, packed 2 bits a base as the device reads it), the reads as ASCII, and per job the
window [rb, re) into the text of 2 l_pac bases (forward strand, then the reverse complement), is_rev (the job aligns the read's reverse
complement) and xtra as mem_matesw sets it: KSW_XSUBO | KSW_XSTART | (KSW_XBYTE where l_ms * a < 250) | min_seed_len * a.  `q` holds the
codes 0..4 the host walk and the reference get.  `must` says what the case is about: name -> function(res), res the int32 [n, 7] rows
{score, te, qe, score2, te2, tb, qb} of the host walk.  A generator that stops producing its edge fails the test that checks `must`.
`overflow` marks the jobs whose byte pass ends at 255: the only ones whose expected result is the reference's first pass alone."""
from __future__ import annotations

import functools
import hashlib
import zlib
from types import SimpleNamespace

import numpy as np

XBYTE, XSTOP, XSUBO, XSTART = 0x10000, 0x20000, 0x40000, 0x80000
DEFAULT = (1, 4, 6, 1, 6, 1)
SCORINGS = ((2, 3, 5, 2, 5, 2), (1, 1, 1, 1, 2, 1), (3, 5, 7, 2, 9, 1), (1, 4, 6, 1, 0, 1), (1, 100, 6, 1, 6, 1))
MIN_SEED_LEN = 19
MSW_SLEN, MSW_JOBS_PER_BLOCK, MSW_TBUF = 40, 8, 64         # csrc/pair_kernels.hip
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 144, 159, 160, 161, 176, 240, 248, 249, 250, 255, 256, 257, 304, 319, 320)
TLENS = (1, 2, 19, 63, 64, 65, 127, 128, 129, 700)
FAMILIES = ("lengths", "mixed_lengths", "mixed_width", "batch_size", "targets", "text_edges", "letters", "ins_cross", "second_best", "ties",
            "threshold", "scorings", "overflow")

_NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _NT4[ord(_c)] = _NT4[ord(_c.lower())] = _i


def nt4(ascii_read):
    """the code of every letter (csrc/pair_kernels.hip: msw_nt4): A C G T in either case, anything else 4"""
    return _NT4[np.frombuffer(bytes(ascii_read), np.uint8)]


def revcomp(x):
    x = np.asarray(x, np.uint8)[::-1]
    return np.where(x < 4, 3 - x, 4).astype(np.uint8)


def to_ascii(codes):
    return np.frombuffer(b"ACGTN", np.uint8)[np.asarray(codes, np.uint8)].tobytes()


def pack_pac(g):
    pad = (-len(g)) % 4
    codes = np.concatenate([g, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    pac = ((codes[:, 0] << 6) | (codes[:, 1] << 4) | (codes[:, 2] << 2) | codes[:, 3]).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([pac, np.zeros(8, np.uint8)]))


def lanes_of(xtra):
    return 16 if xtra & XBYTE else 8


def slen_of(l_ms, xtra):
    return (l_ms + lanes_of(xtra) - 1) // lanes_of(xtra)


def xtra_of(l_ms, scoring, minsc=None):
    a = scoring[0]
    return XSUBO | XSTART | (XBYTE if l_ms * a < 250 else 0) | (MIN_SEED_LEN * a if minsc is None else minsc)


def other(c, k=2):
    """a base that differs from c"""
    return (np.asarray(c, np.uint8) + k) & 3


class Batch:
    """the jobs of one case, in order.  A target given as codes is appended to the case's genome (every fifth one as its reverse complement, so that the
    window lies on the reverse half of the text); a window is taken as it is."""

    def __init__(self, name, family, scoring=DEFAULT, genome=None):
        self.name, self.family, self.scoring = name, family, tuple(scoring)
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.fixed = None if genome is None else np.ascontiguousarray(genome, dtype=np.uint8)
        self.pieces, self.at, self.jobs = [], 0, []

    def rand(self, n):
        return self.rng.integers(0, 4, size=int(n)).astype(np.uint8)

    def add(self, q, target=None, window=None, is_rev=None, rev_half=None, ascii_read=None, overflow=False, tag=""):
        """q: the codes the alignment gets (None with ascii_read: derived from the letters) -> the job's index"""
        k = len(self.jobs)
        is_rev = (k & 1) if is_rev is None else int(is_rev)
        if ascii_read is None:
            q = np.ascontiguousarray(q, dtype=np.uint8)
            ascii_read = to_ascii(revcomp(q) if is_rev else q)
        else:
            c = nt4(ascii_read)
            q = np.ascontiguousarray(revcomp(c) if is_rev else c)
        if window is None:
            assert self.fixed is None
            target = np.ascontiguousarray(target, dtype=np.uint8)
            assert len(target) and target.max() < 4
            rev_half = (k % 5 == 3) if rev_half is None else rev_half
            self.pieces += [revcomp(target) if rev_half else target, self.rand(3)]
            window = (self.at, len(target), rev_half)
            self.at += len(target) + 3
        else:
            assert self.fixed is not None
            window = (int(window[0]), int(window[1]) - int(window[0]), None)
        self.jobs.append(SimpleNamespace(q=q, ascii=bytes(ascii_read), is_rev=is_rev, window=window, overflow=bool(overflow), tag=tag))
        return k

    def case(self, must):
        g = self.fixed if self.fixed is not None else np.concatenate(self.pieces)
        l_pac = len(g)
        n = len(self.jobs)
        rb, re = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for k, j in enumerate(self.jobs):
            p, ln, rev = j.window
            rb[k] = 2 * l_pac - (p + ln) if rev else p
            re[k] = rb[k] + ln
        assert (rb >= 0).all() and (re <= 2 * l_pac).all() and (re > rb).all()
        l_ms = np.array([len(j.q) for j in self.jobs], np.int32)
        xtra = np.array([xtra_of(int(l), self.scoring) for l in l_ms], np.int32)
        offs = np.concatenate([[0], np.cumsum(l_ms)]).astype(np.uint32)
        c = SimpleNamespace(name=self.name, family=self.family, scoring=self.scoring, genome=g, pac=pack_pac(g), l_pac=l_pac, n=n,
                            reads=np.frombuffer(b"".join(j.ascii for j in self.jobs), np.uint8).copy(), offs=offs, l_ms=l_ms,
                            is_rev=np.array([j.is_rev for j in self.jobs], np.int32), rb=rb, re=re, xtra=xtra, q=[j.q for j in self.jobs],
                            overflow=np.array([j.overflow for j in self.jobs], bool), tags=[j.tag for j in self.jobs], must=dict(must))
        assert c.must and (not c.overflow.any() or self.family == "overflow")
        for k in range(n):                                        # every job is one the device takes (bmh_matesw_device_takes)
            assert 0 < l_ms[k] and slen_of(int(l_ms[k]), int(xtra[k])) <= MSW_SLEN and 0 < re[k] - rb[k] < 65536, (self.name, k)
        return c


def text_of(c):
    """the 2 l_pac bases the windows of a case are cut from"""
    return np.concatenate([c.genome, 3 - c.genome[::-1]]).astype(np.uint8)


def target_of(c, k, text=None):
    text = text_of(c) if text is None else text
    return np.ascontiguousarray(text[c.rb[k]:c.re[k]])


def reference_rows(ref, c):
    """oracle_py.Ref.align2, the reference's ksw_align2, on every job of a case.  A job of the overflow family that is marked is called without KSW_XSTART: its
    first pass alone, which ends at 255 -- the second would run over an empty query and read in front of the reference's arrays."""
    text = text_of(c)
    out = np.zeros((c.n, 7), np.int32)
    for k in range(c.n):
        out[k] = ref.align2(c.q[k], target_of(c, k, text), c.scoring, int(c.xtra[k]) & ~(XSTART if c.overflow[k] else 0))
    return out


def edited(s, subs=(), n_at=None, ins=None, dele=None):
    """the query for a stretch s of the text: substitutions, an N, k inserted bases in front of position p, k bases removed from position p on"""
    q = np.array(s, np.uint8)
    for p in subs:
        q[p] = (q[p] + 1 + p % 3) & 3
    if n_at is not None:
        q[n_at] = 4
    if dele is not None:
        p, k = dele
        q = np.concatenate([q[:p], q[p + k:]])
    if ins is not None:
        p, k = ins
        # inserted bases that continue neither side: the base the text has behind them, nor the one in front
        z = min(set(range(4)) - {int(q[p - 1]), int(q[min(p, len(q) - 1)])})
        x = np.full(k, z, np.uint8)
        q = np.concatenate([q[:p], x, q[p:]])
    return np.ascontiguousarray(q)


def in_window(b, s, left=None, right=None):
    left = int(b.rng.integers(5, 80)) if left is None else left
    right = int(b.rng.integers(5, 80)) if right is None else right
    return np.concatenate([b.rand(left), s, b.rand(right)])


def add_variants(b, L, n_var=4):
    """the jobs of one query length: exact, substitutions and an N, an insertion, a deletion -- wherever the length allows"""
    a = b.scoring[0]
    for v in range(n_var):
        if v == 0:
            s = b.rand(L)
            q = edited(s, subs=[L // 2] if L * a == 255 else [])       # (a word-mode 255 is kept for the overflow family's byte passes)
        elif v == 1:
            s = b.rand(L)
            q = edited(s, subs=[L // 3, 2 * L // 3] if L >= 8 else [], n_at=L // 2 if L >= 4 else None)
        elif v == 2:
            s = b.rand(L - 2 if L >= 31 else L)
            q = edited(s, ins=(L // 2, 2)) if L >= 31 else s.copy()
        else:
            s = b.rand(L + 2 if L >= 31 else L)
            q = edited(s, dele=(L // 2, 2)) if L >= 31 else edited(s, subs=[0] if L >= 2 else [])
        assert len(q) == L
        b.add(q, in_window(b, s), tag=f"len{L}v{v}")


def found(res, k=None):
    """the jobs whose mate was found with its start"""
    r = res if k is None else res[k:k + 1]
    return (r[:, 0] >= MIN_SEED_LEN) & (r[:, 5] >= 0) & (r[:, 6] >= 0)


# ---------------------------------------------------------------------------------------------------------------- the families

def _lengths():
    out = []
    for L in LENGTHS:
        b = Batch(f"len_{L}", "lengths")
        add_variants(b, L)
        must = {"the length": lambda res, L=L, b=b: all(len(j.q) == L for j in b.jobs)}
        if L >= 31:
            must["the mate is found with its start"] = lambda res, L=L: found(res if L >= 144 else res[[0, 2, 3]]).all()
            must["the exact mate scores its length"] = lambda res, L=L: res[0, 0] == (L if L != 255 else L - 5) and res[0, 2] == L - 1
            must["insertion and deletion are taken"] = lambda res, L=L: res[2, 0] == L - 2 - 8 and res[3, 0] == L - 8
        else:
            must["below the threshold no start is computed"] = lambda res, L=L: (res[:, 0] <= L).all() and (L >= 19 or (res[:, 5:] == -1).all())
        out.append(b.case(must))
    return out


def _mixed_lengths():
    out = []
    for name, ls in (("mixed_37_100_150_160", (37, 100, 150, 160)), ("mixed_161_to_249", (161, 177, 200, 249))):
        b = Batch(name, "mixed_lengths")
        for i in range(16):
            L = ls[i % 4]
            s = b.rand(L - 2 if i % 3 == 1 else L)
            b.add(edited(s, subs=[L // 4] if i % 2 else [], ins=(L // 2, 2) if i % 3 == 1 else None), in_window(b, s))
        out.append(b.case({
            "every wave holds the four lengths": lambda res, b=b, ls=ls: all(tuple(len(j.q) for j in b.jobs[w:w + 4]) == ls for w in range(0, 16, 4)),
            "three or four different columns per wave": lambda res, b=b: len({slen_of(len(j.q), XBYTE) for j in b.jobs[:4]}) >= 3,
            "found": lambda res: found(res).all()}))
    return out


def _mixed_width():
    b = Batch("mixed_249_250", "mixed_width")
    for i in range(8):
        L = 249 + (i & 1)
        s = b.rand(L)
        b.add(edited(s, subs=[10 + i, 200] if i >= 2 else [L // 2]), in_window(b, s))
    out = [b.case({"byte and word jobs alternate": lambda res, b=b: [lanes_of(xtra_of(len(j.q), DEFAULT)) for j in b.jobs] == [16, 8] * 4,
                   "found": lambda res: found(res).all(),
                   "no word-mode 255": lambda res: (res[:, 0] != 255).all()})]
    # a byte job of 40 bases has 8 padding columns, in word mode it would have none: the second copy that ends on the band's edge and is seen two rows on
    # through the padding (second_best_band_padding) in a wave with a word job
    b = Batch("mixed_40_260", "mixed_width")
    for off in (40, 41, 40):
        mate = b.rand(40)
        b.add(mate, _sb_target(b, 400, 200, mate, [(200 + off, 20)]), rev_half=False)
    s = b.rand(260)
    b.add(edited(s, subs=[100, 200]), in_window(b, s))
    out.append(b.case({"widths": lambda res, b=b: [lanes_of(xtra_of(len(j.q), DEFAULT)) for j in b.jobs] == [16, 16, 16, 8],
                       "seen through the padding": lambda res: [tuple(r[[0, 3, 4]]) for r in res[:3]] == [(40, 20, 242), (40, 20, 241), (40, 20, 242)],
                       "found": lambda res: found(res).all()}))
    return out


def _batch_size():
    out = []
    for n in (1, 3, 4, 5, 8, 9):
        b = Batch(f"batch_of_{n}", "batch_size")
        for i in range(n):
            s = b.rand(40 + 7 * i)
            b.add(edited(s, subs=[20] if i & 1 else []), in_window(b, s))
        out.append(b.case({"jobs": lambda res, n=n: len(res) == n, "found": lambda res: found(res).all()}))
    return out


def _targets():
    out = []
    b = Batch("tlen_edges", "targets")
    s = b.rand(30)
    want = []
    for T in TLENS:
        b.add(s, np.concatenate([b.rand(T - 30), s]) if T >= 30 else s[-T:], tag=f"tlen{T}, mate at the end")
        want.append((T, min(T, 30), T - 1))
    for T in TLENS:
        if T >= 63:
            b.add(s, np.concatenate([s, b.rand(T - 30)]), tag=f"tlen{T}, mate at the start")
            want.append((T, 30, 29))
    out.append(b.case({
        "window lengths": lambda res, b=b, want=want: [j.window[1] for j in b.jobs] == [w[0] for w in want],
        "score and last row": lambda res, want=want: all(res[k, 0] == w[1] and res[k, 1] == w[2] for k, w in enumerate(want)),
        "a start from 19 rows on": lambda res, want=want: all((res[k, 5] >= 0) == (w[1] >= 19) for k, w in enumerate(want))}))
    b = Batch("tlen_5_beside_700", "targets")
    s = b.rand(60)
    for i in range(8):
        b.add(s, s[-5:] if i in (1, 6) else np.concatenate([b.rand(640), s]), rev_half=False)
    out.append(b.case({"short and long windows in one wave": lambda res: [int(r[1]) for r in res] == [699, 4, 699, 699, 699, 699, 4, 699],
                       "scores": lambda res: [int(r[0]) for r in res] == [60, 5, 60, 60, 60, 60, 5, 60]}))
    # rows beyond 2^15 and 2^16 - 2^14 in the 16-bit row of a bookkeeping word
    b = Batch("tlen_65535", "targets")
    s = b.rand(150)
    s2 = edited(s, subs=[30, 75, 120])
    for first, second in ((s, s2), (s2, s)):
        t = b.rand(65535)
        t[40100:40250] = first; t[60200:60350] = second
        b.add(s, t, is_rev=0, rev_half=False)
    out.append(b.case({
        "the mate beyond row 40000, its second copy beyond 60000": lambda res: res[0, 0] == 150 and res[0, 1] == 40249 and res[0, 3] == 135 and res[0, 4] == 60349,
        "and the other way round": lambda res: res[1, 0] == 150 and res[1, 1] == 60349 and res[1, 3] == 135 and res[1, 4] == 40249,
        "starts": lambda res: res[0, 5] == 40100 and res[1, 5] == 60200 and (res[:, 6] == 0).all()}))
    return out


def _text_edges():
    out = []
    for l_pac in (1001, 1002, 1003):
        g = np.random.default_rng(l_pac).integers(0, 4, size=l_pac).astype(np.uint8)
        b = Batch(f"text_edges_{l_pac}", "text_edges", genome=g)
        text = np.concatenate([g, 3 - g[::-1]]).astype(np.uint8)
        wins = [(l_pac - 120, l_pac), (l_pac, l_pac + 120), (2 * l_pac - 120, 2 * l_pac), (l_pac - 60, l_pac + 60), (l_pac + 300, l_pac + 500), (0, 90),
                (l_pac - 1, l_pac), (2 * l_pac - 1, 2 * l_pac)]
        for k, (w0, w1) in enumerate(wins):
            ln = min(50, w1 - w0)
            at_end = k in (0, 2, 3, 6, 7)                           # the mate's last base is the window's last
            s = text[w1 - ln:w1] if at_end else text[w0:w0 + ln]
            q = edited(s, subs=[ln // 2] if k & 1 and ln > 1 else [])
            if ln == 1:
                q = np.concatenate([np.repeat(other(s), 20), s])    # one row: the last base of the text against 21 columns, the last of them its match
            b.add(q, window=(w0, w1), is_rev=(k >> 1) & 1)
        out.append(b.case({
            "the genome's length modulo 4": lambda res, l_pac=l_pac: l_pac % 4 == l_pac - 1000,
            "windows that end at l_pac, begin there and reach 2 l_pac": lambda res, b=b, l=l_pac: [(j.window[0], j.window[0] + j.window[1]) for j in b.jobs[:3]] == [(l - 120, l), (l, l + 120), (2 * l - 120, 2 * l)],
            "the mate on the window's last base": lambda res: res[0, 1] == 119 and res[2, 1] == 119 and res[3, 1] == 119,
            "found": lambda res: found(res[:6]).all(),
            "the text's last bases alone": lambda res: (res[6:, 0] == 1).all() and (res[6:, 1] == 0).all() and (res[6:, 2] == 20).all()}))
    return out


def _letters():
    b = Batch("letters", "letters")
    alphabet = b"acgtnNRYKMSWBDHVryUu.-*"
    for i in range(12):
        s = b.rand(60 + i)
        is_rev = i & 1
        read = bytearray(to_ascii(revcomp(s) if is_rev else s))
        for p in range(i % 3, len(read), 3):                       # every third letter in lower case
            read[p] = read[p] | 0x20
        for u, p in enumerate((7, 23, 41 + i)):                    # three letters that are no base
            read[p] = alphabet[4 + (3 * i + u) % (len(alphabet) - 4)]
        b.add(None, in_window(b, s), is_rev=is_rev, ascii_read=bytes(read))
    return [b.case({
        "lower case, N, n and IUPAC letters": lambda res, b=b: all(any(x in j.ascii for x in b"acgt") for j in b.jobs) and {x for j in b.jobs for x in j.ascii} >= set(b"NnRYKMSWBDHV"),
        "three codes 4 per read, the rest bases": lambda res, b=b: all((j.q == 4).sum() == 3 for j in b.jobs),
        "found on both strands": lambda res: found(res).all() and (res[:, 0] >= 40).all()})]


def _ins_cross():
    """an insertion of k bases whose first base is the first column of lane L + 1 (k = 1) or the last column of lane L: its F leaves lane L"""
    out = []
    for scoring, sname in ((DEFAULT, "default"), ((1, 4, 6, 1, 2, 1), "o2")):
        for slen, qlen in ((10, 160), (16, 249)):
            for extra in ((False, True) if (slen == 10 and sname == "default") else (False,)):
                b = Batch(f"ins_cross_{slen}_{sname}" + ("_beside_37" if extra else ""), "ins_cross", scoring)
                want = []
                if extra:                                          # a shorter job in the first wave: the row with a test per column
                    s = b.rand(37); b.add(s, in_window(b, s), rev_half=False); want.append(None)
                for lane in (0, 1, 7, 14):
                    for k in (1, 2, 3, 4):
                        p = (lane + 1) * slen - (0 if k == 1 else 1)
                        s = b.rand(qlen - k)
                        q = edited(s, ins=(p, k))
                        b.add(q, in_window(b, s, 12, 12), rev_half=False)
                        cost = scoring[4] + k * scoring[5]
                        want.append((max(qlen - k - cost, p, qlen - k - p), qlen - k - cost > max(p, qlen - k - p), lane))
                out.append(b.case({
                    "columns per lane": lambda res, b=b, slen=slen, extra=extra: all(slen_of(len(j.q), XBYTE) == slen for j in b.jobs[extra:]),
                    "scores": lambda res, want=want: all(w is None or res[i, 0] == w[0] for i, w in enumerate(want)),
                    "the insertion is the best path out of each of the four lanes (cheap opens: three times or more)": lambda res, want=want, sname=sname:
                        all(sum(1 for w in want if w and w[1] and w[2] == lane) >= (3 if sname == "o2" else 1) for lane in (0, 1, 7, 14))}))
    return out


def _sb_target(b, total, te, mate, copies):
    """random rows, the mate ending at row te, and (end row, n) copies of the mate's last n bases; the base in front of a copy does not continue it"""
    t = b.rand(total)
    t[te - len(mate) + 1:te + 1] = mate
    for e, n in copies:
        t[e - n] = other(mate[-n - 1], 1)
        t[e - n + 1:e + 1] = mate[-n:]
    return t


def _second_best():
    out = []
    # the second copy (the mate's last 20 bases, exact) at the four rows around the band te +- d
    # (mates of 48 bases fill their 16 lanes; "padding": one of 40 leaves 8 columns that score 0 against everything -- a 20 at the query's end walks on through
    # them for 7 rows, and as a row is "consecutive" only to the row of its entry's maximum, every second of those rows opens an entry: the copy that ends ON the
    # band's edge is seen two rows further out)
    for scoring, n, sub, what in ((DEFAULT, 48, None, "a1"), ((2, 3, 5, 2, 5, 2), 48, None, "a2"), ((3, 5, 7, 2, 9, 1), 48, 24, "a3"), (DEFAULT, 40, None, "padding")):
        a, bmis = scoring[0], scoring[1]
        score = n * a if sub is None else (n - 1) * a - bmis
        d = -(-score // a)
        b = Batch(f"second_best_band_{what}", "second_best", scoring)
        te, want = 200, []
        for off in (-d - 1, -d, d, d + 1):
            if off < 0 and -off < n:
                continue                                            # (that row lies inside the mate's own rows)
            mate = b.rand(n)
            q = mate if sub is None else edited(mate, subs=[sub])
            b.add(q, _sb_target(b, 400, te, mate, [(te + off, 20)]), rev_half=False)
            want.append((te + off + (2 if what == "padding" and off == d else 0), abs(off) > d or (what == "padding" and off == d)))
        out.append(b.case({
            "the band is d = ceil(score / a) rows": lambda res, score=score, d=d, a=a, sub=sub: (res[:, 0] == score).all() and (res[:, 1] == 200).all() and d == -(-score // a) and (sub is None or score % a != 0),
            "score2 is set exactly outside the band": lambda res, want=want, a=a: all((res[i, 3] == 20 * a and res[i, 4] == e) if outside else (res[i, 3] == -1 and res[i, 4] == -1) for i, (e, outside) in enumerate(want)),
            "both sides of an edge are here": lambda res, want=want: {o for _, o in want} == {True, False}}))
    b = Batch("second_best_copies", "second_best")
    mate = b.rand(40)
    p20, p25 = 20, 25
    b.add(mate, _sb_target(b, 500, 300, mate, [(100, p20), (170, p20)]), tag="two equal second bests in front: the first")
    b.add(mate, _sb_target(b, 500, 200, mate, [(100, p20), (400, p20)]), tag="one on either side: the first")
    b.add(mate, _sb_target(b, 500, 200, mate, [(100, p20), (400, p25)]), tag="three copies: the better one behind")
    b.add(mate, _sb_target(b, 500, 200, mate, [(100, p25), (400, p20)]), tag="three copies: the better one in front")
    # a tandem stretch: 24 copies of the last 20 bases, two rows apart -- 24 open entries for one job, every lane scans two
    tand = [(30 + 22 * i, p20) for i in range(24)]
    b.add(mate, _sb_target(b, 700, 650, mate, tand), tag="tandem, all equal: the first entry")
    b.add(mate, _sb_target(b, 700, 650, mate, tand[:19] + [(30 + 22 * 19 + 5, p25)] + tand[21:]), tag="tandem, the best is entry 19")
    # two paths that reach 25 on consecutive rows: one entry, at the first of the two rows
    T = b.rand(26)
    M = b.rand(40)
    q = np.concatenate([T[:25], other(T[25:26]), M, other(T[0:1]), T[1:]])
    t = b.rand(400); t[100:126] = T; t[250:290] = M
    b.add(q, t, tag="plateau")
    out.append(b.case({
        "the first of equals": lambda res: (res[:2, 3] == 20).all() and (res[:2, 4] == 100).all(),
        "the better of three": lambda res: (res[2:4, 3] == 25).all() and res[2, 4] == 400 and res[3, 4] == 100,
        "more than 16 entries": lambda res: res[4, 3] == 20 and res[4, 4] == 30 and res[5, 3] == 25 and res[5, 4] == 30 + 22 * 19 + 5,
        "rows that follow each other keep one entry, at the first row of their maximum": lambda res: res[6, 0] == 40 and res[6, 3] == 25 and res[6, 4] == 124,
        "the best": lambda res: (res[:, 0] == 40).all()}))
    return out


def _once(b, u, left, right):
    """u once in a window whose bases beside it continue neither the u in front of it in the query nor the one behind"""
    t = np.concatenate([b.rand(left), u, b.rand(right)])
    t[left - 1], t[left + len(u)] = other(u[-1], 1), other(u[0], 1)
    return t


def _ties():
    b = Batch("ties", "ties")
    u = b.rand(30)
    for i in range(2):
        b.add(np.concatenate([u, u]), _once(b, u, 40 + i, 40), is_rev=i)
    m = b.rand(50)
    for i in range(2):
        t = b.rand(400); t[100:150] = m; t[250 + i:300 + i] = m
        b.add(m, t, is_rev=i)
    out = [b.case({
        "the smaller query end of two": lambda res: (res[:2, 2] == 29).all() and (res[:2, 0] == 30).all() and (res[:2, 6] == 0).all(),
        "the first target row of two": lambda res: (res[2:4, 1] == 149).all() and (res[2:4, 0] == 50).all() and res[2, 3] == 50 and res[2, 4] == 299 and res[3, 4] == 300})]
    # the same with columns of 15 and 13 segments, and with a word-mode mate (the second copy lies beyond the rows the first one's gap keeps above the threshold)
    for name, nu, nm in (("ties_long", 120, 200), ("ties_word", 130, 260)):
        b = Batch(name, "ties")
        u = b.rand(nu)
        b.add(np.concatenate([u, u]), _once(b, u, 40, 40))
        m = b.rand(nm)
        t = b.rand(1300); t[50:50 + nm] = m; t[900:900 + nm] = m
        b.add(m, t)
        out.append(b.case({
            "the smaller query end of two": lambda res, nu=nu: res[0, 0] == nu and res[0, 2] == nu - 1 and res[0, 6] == 0,
            "the first target row of two": lambda res, nm=nm: res[1, 0] == nm and res[1, 1] == 49 + nm and res[1, 3] == nm and res[1, 4] == 899 + nm,
            "the width": lambda res, b=b, name=name: all((lanes_of(xtra_of(len(j.q), DEFAULT)) == 8) == (name == "ties_word") for j in b.jobs)}))
    return out


def _threshold():
    out = []
    for scoring in (DEFAULT, SCORINGS[0], SCORINGS[2]):
        a = scoring[0]
        b = Batch(f"threshold_a{a}", "threshold", scoring)
        for n in (18, 19, 18, 19):
            q = b.rand(50)
            t = other(q)                                            # every base of the main diagonal mismatches,
            t[16:16 + n] = q[16:16 + n]                             # but for n of them
            b.add(q, np.concatenate([b.rand(30), t, b.rand(30)]))
        for i in range(4):
            b.add(b.rand(60 + i), b.rand(200 + 9 * i), tag="no mate in the window")
        out.append(b.case({
            "minsc - 1: no start": lambda res, a=a: all(res[k, 0] == 18 * a and res[k, 5] == -1 and res[k, 6] == -1 for k in (0, 2)),
            "minsc: a start": lambda res, a=a: all(res[k, 0] == 19 * a and res[k, 5] == 46 and res[k, 6] == 16 for k in (1, 3)),
            "nothing in a window without the mate": lambda res, a=a: (res[4:, 0] < 19 * a).all() and (res[4:, 3:] == -1).all()}))
    return out


def _scorings():
    out = []
    for scoring in SCORINGS:
        a = scoring[0]
        wide = (250 + a - 1) // a                                   # the shortest word-mode mate
        top = min(wide - 1, (254 - scoring[1]) // a)                # the longest byte-mode mate (that cannot overflow)
        for width, ls in (("byte", (60, min(100, top - 3), top - 1, top)), ("word", (wide, wide + 1, 150 if wide < 140 else 280, 300))):
            b = Batch("scoring_" + "_".join(map(str, scoring)) + "_" + width, "scorings", scoring)
            for L in ls:
                add_variants(b, L)
            out.append(b.case({
                "the width": lambda res, b=b, a=a, width=width: all((len(j.q) * a < 250) == (width == "byte") for j in b.jobs),
                "the class limit": lambda res, ls=ls, top=top, wide=wide, width=width: (top if width == "byte" else wide) in ls,
                "found": lambda res, a=a: (res[:, 0] >= 19 * a).all() and (res[:, 5] >= 0).sum() >= len(res) - 2,
                "no 255": lambda res: (res[:, 0] != 255).all()}))
    return out


def _overflow():
    """the byte pass ends with 255 at the row where gmax + shift >= 255, shift = max(b, 1): an exact mate of n bases overflows from n * a + b >= 255 on"""
    out = []
    # ((1, 99, ...): b just inside the register forms' gate, columns of ten)
    for scoring in ((1, 6, 6, 1, 6, 1), (1, 9, 6, 1, 6, 1), (2, 8, 5, 2, 5, 2), (1, 100, 6, 1, 6, 1), (1, 99, 6, 1, 6, 1)):
        a, bmis = scoring[0], scoring[1]
        n_over = -(-(255 - bmis) // a)                              # the shortest exact mate that overflows
        assert n_over * a < 250 and (n_over - 1) * a + bmis < 255 <= n_over * a + bmis
        b = Batch("overflow_" + "_".join(map(str, scoring)), "overflow", scoring)
        fits, over = [], []
        for L, ov in ((n_over - 1, False), (n_over, True), (n_over - 1, False), (n_over, True)):
            s = b.rand(L)
            k = b.add(s, in_window(b, s, 60, 60), overflow=ov, rev_half=False, tag="exact")
            (over if ov else fits).append((k, L))
        # near-exact: a substitution three bases from the end leaves n_over - 4 matches in a row: it fits; a longer mate with one N in front overflows at the same row
        s = b.rand(n_over)
        k_near = b.add(edited(s, subs=[n_over - 4]), in_window(b, s, 60, 60), rev_half=False, tag="near-exact, fits")
        k_more = None
        if (n_over + 4) * a < 250:
            s = b.rand(n_over + 4)
            k_more = b.add(edited(s, n_at=2), in_window(b, s, 60, 60), overflow=True, rev_half=False, tag="near-exact, overflows")
        # an exact mate longer than it takes: the pass ends at the row that reaches 255, not at the mate's last
        k_long = None
        if (n_over + 1) * a < 250:
            s = b.rand(min(n_over + 4, 249 // a))
            k_long = b.add(s, in_window(b, s, 60, 60), overflow=True, rev_half=False, tag="exact, longer")
        # one overflow beside three ordinary jobs in a wave
        while len(b.jobs) % 4:
            s = b.rand(50); b.add(s, in_window(b, s), rev_half=False)
        w0 = len(b.jobs)
        for i in range(4):
            s = b.rand(n_over if i == 2 else 70 + i)
            b.add(s, in_window(b, s, 60, 60), overflow=i == 2, rev_half=False)
        out.append(b.case({
            "the longest mate that fits": lambda res, fits=fits, a=a: all(res[k, 0] == L * a < 255 and res[k, 1] == 60 + L - 1 and res[k, 5] == 60 for k, L in fits),
            "the shortest that overflows": lambda res, over=over: all(tuple(res[k]) == (255, 60 + L - 1, -1, -1, -1, -1, -1) for k, L in over),
            "near-exact": lambda res, k_near=k_near, k_more=k_more, n_over=n_over: 0 < res[k_near, 0] < 255 and res[k_near, 5] >= 0 and (k_more is None or tuple(res[k_more, [0, 2, 5, 6]]) == (255, -1, -1, -1)),
            "the pass ends where 255 is reached": lambda res, k_long=k_long, n_over=n_over, a=a, bmis=bmis: k_long is None or (n_over * a + bmis == 255 and tuple(res[k_long]) == (255, 60 + n_over - 1, -1, -1, -1, -1, -1)),
            "one overflow in a wave of ordinary jobs": lambda res, w0=w0: tuple(res[w0 + 2, [0, 2, 5, 6]]) == (255, -1, -1, -1) and found(res[[w0, w0 + 1, w0 + 3]]).all(),
            "marked": lambda res, b=b: ((res[:, 0] == 255) == np.array([j.overflow for j in b.jobs])).all()}))
    # byte and word jobs in one batch, one of the byte jobs overflowing
    b = Batch("overflow_mixed_width", "overflow", (1, 9, 6, 1, 6, 1))
    for L, ov in ((246, True), (250, False), (245, False), (256, False)):
        s = b.rand(L)
        b.add(edited(s, subs=[L // 2] if L == 256 else []), in_window(b, s, 60, 60), overflow=ov, rev_half=False)
    out.append(b.case({
        "widths": lambda res, b=b: [lanes_of(xtra_of(len(j.q), b.scoring)) for j in b.jobs] == [16, 8, 16, 8],
        "the byte job overflows, the word job beside it scores more": lambda res: tuple(res[0]) == (255, 305, -1, -1, -1, -1, -1) and res[1, 0] == 250 and res[2, 0] == 245 and found(res[1:]).all()}))
    return out


@functools.lru_cache(maxsize=1)
def all_cases():
    cases = {}
    for fam in (_lengths, _mixed_lengths, _mixed_width, _batch_size, _targets, _text_edges, _letters, _ins_cross, _second_best, _ties, _threshold,
                _scorings, _overflow):
        for c in fam():
            assert c.name not in cases
            cases[c.name] = c
    return cases


def names():
    return tuple(all_cases())


def get(name):
    return all_cases()[name]


def job_slices():
    """case name -> the rows of its jobs in the fixture (the jobs of all cases in table order)"""
    out, at = {}, 0
    for name, c in all_cases().items():
        out[name] = slice(at, at + c.n)
        at += c.n
    return out


def digest():
    """of everything a result depends on: genomes, reads, windows, flags and scorings of every job in table order"""
    h = hashlib.sha256()
    for name, c in all_cases().items():
        h.update(name.encode()); h.update(np.array(c.scoring, np.int32).tobytes()); h.update(c.genome.tobytes()); h.update(c.reads.tobytes())
        for arr in (c.offs, c.l_ms, c.is_rev, c.rb, c.re, c.xtra, c.overflow.astype(np.uint8)):
            h.update(np.ascontiguousarray(arr).tobytes())
        for q in c.q:
            h.update(q.tobytes())
    return h.hexdigest()


def refusals():
    """batches bmh_matesw_batch_device must refuse: (what, the job that is not taken, l_ms, tlen, word mode).  The other jobs of the batch are ordinary."""
    return (("l_ms 321 in word mode", 2, 321, 400, True), ("l_ms 0", 0, 0, 100, False), ("tlen 0", 3, 50, 0, False), ("tlen 65536", 1, 50, 65536, False))
