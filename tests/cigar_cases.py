"""Hand-made regions for the CIGAR stage (csrc/cigar_kernels.hip against oracle/cigar_oracle.c and the reference's mem_reg2aln): every job kind of
cigar_classify_kernel at its limits, the band retry of mem_reg2aln and the demotion out of cigar_dp16_kernel, every wave-per-region instantiation from
both sides of its query length, the traceback windows of cigar_finish_kernel, the NM / MD loops at their chunk edges, the edges of the 2-bit text, the
long form, the CIGAR and MD slots, and the scorings with a positive gap extension.  Plain numpy, no tests, no GPU.

One small genome serves all jobs.  A job is one region of one read: the read as ASCII, [qb, qe) in it, [rb, re) in the text of 2 l_pac bases (forward strand,
then its reverse complement), the local score truesc and the band reg_w the region carries.  A job is written in the coordinates of the DP: target T and
query Q as ksw_global2 sees them, after bwa_gen_cigar2 reversed both for a region on the reverse strand.  A batch is a scoring, opt_w, a record stride and
its jobs in order.

The routing is restated here from the code: g_infer_bw, cg_first_w2, the w / n_col rule, the kind thresholds, need = ceil(qlen / 64), is_long.  Every job
asserts the (w2, w, n_col, kind) it was built for when the table is made, so that an edit cannot slide a job off its limit silently; `limits` names what a
job is in the table for (tests/test_cigar_cases.py asserts by name that every limit is there from both sides, on both strands)."""
from __future__ import annotations

import functools
import hashlib
import zlib
from types import SimpleNamespace

import numpy as np

L_PAC = 20003                                                     # not a multiple of 4: the last byte of the packed text is partly filled
DEFAULT = (1, 4, 6, 1, 6, 1)
# tests/test_extension_scoring.py: SCORINGS with e > 0 (the band inference divides by e)
SCORINGS = {"default": (1, 4, 6, 1, 6, 1), "scaled2": (2, 8, 12, 2, 12, 2), "ins_dear": (1, 4, 6, 1, 9, 3), "del_dear": (1, 4, 9, 3, 6, 1),
            "lut_edge": (3, 31, 9, 3, 9, 3), "generic": (33, 40, 50, 7, 50, 7), "b0": (1, 0, 6, 1, 6, 1), "free_open": (1, 4, 0, 1, 0, 1)}
CG_LDS_MAX = 704                                                  # csrc/cigar_kernels.hip
KINDS = ("reject", "trivial", "F2", "F3", "F5", "F10", "F16", "slow")
KIND_COLS = (("F2", 32), ("F3", 48), ("F5", 80), ("F10", 160), ("F16", 256))
SLOW_FORMS = ((1, "1,0"), (2, "2,1"), (3, "3,2"), (5, "5,3"), (8, "8,5"), (11, "11,8"))      # cigar_kernel<C, CLO>: CLO < need <= C
FAMILIES = ("kinds", "retry", "trace", "geometry", "slots", "scorings")
HOMOPOLYMER, DINUC = 6000, 6100                                   # planted: AAAAAAAA and ACACACACAC, for the placements of equal cost


def _genome():
    g = np.random.default_rng(20003).integers(0, 4, size=L_PAC).astype(np.uint8)
    g[HOMOPOLYMER - 1], g[HOMOPOLYMER:HOMOPOLYMER + 8], g[HOMOPOLYMER + 8] = 1, 0, 2
    g[DINUC - 1], g[DINUC:DINUC + 10], g[DINUC + 10] = 3, np.array([0, 1] * 5, np.uint8), 2
    return g


def pack_pac(g):
    """2 bits a base as the kernels read it: pac[f >> 2] >> ((~f & 3) << 1)"""
    pad = (-len(g)) % 4
    codes = np.concatenate([g, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    pac = ((codes[:, 0] << 6) | (codes[:, 1] << 4) | (codes[:, 2] << 2) | codes[:, 3]).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([pac, np.zeros(8, np.uint8)]))


GENOME = _genome()
PAC = pack_pac(GENOME)
TEXT = np.concatenate([GENOME, 3 - GENOME[::-1]]).astype(np.uint8)
GENOME.setflags(write=False); PAC.setflags(write=False); TEXT.setflags(write=False)


def to_ascii(codes):
    return np.frombuffer(b"ACGTN", np.uint8)[np.asarray(codes, np.uint8)].tobytes()


# ---------------------------------------------------------------------------------------------------------------- the routing, restated

def infer_bw(l1, l2, score, a, q, r):
    """g_infer_bw (src/bwamem.c: infer_bw)"""
    d = abs(l1 - l2)
    if l1 == l2 and l1 * a - score < (q + r - a) << 1:
        return 0
    w = int(float(min(l1, l2) * a - score - q) / r + 2.)
    return max(w, d)


def first_w2(scoring, opt_w, qlen, rlen, truesc, reg_w):
    """cg_first_w2: the band of the first round"""
    a, _, od, ed, oi, ei = scoring
    w2 = max(infer_bw(qlen, rlen, truesc, a, oi, ei), infer_bw(qlen, rlen, truesc, a, od, ed))
    if w2 > opt_w:
        w2 = min(w2, reg_w)
    return min(w2, opt_w << 2)


def band_of(scoring, qlen, rlen, w2):
    """the w / n_col rule of bwa_gen_cigar2 for the band w2 of a round -> (w, n_col), or None where no DP runs (one M run)"""
    a, _, od, ed, oi, ei = scoring
    if qlen == rlen and w2 == 0:
        return None
    max_ins = int(float(((qlen + 1) >> 1) * a - oi) / ei + 1.)
    max_del = int(float(((qlen + 1) >> 1) * a - od) / ed + 1.)
    max_gap = max(max_ins, max_del, 1)
    diff = abs(rlen - qlen)
    w = max(min((max_gap + diff + 1) >> 1, w2), diff + 3)
    return w, min(qlen, 2 * w + 1)


def rejected(qb, qe, rb, re):
    return qe - qb <= 0 or rb >= re or (rb < L_PAC and re > L_PAC)


def route(scoring, opt_w, qb, qe, rb, re, truesc, reg_w):
    """cigar_classify_kernel -> (w2, w, n_col, kind)"""
    if rejected(qb, qe, rb, re):
        return (0, 0, 0, "reject")
    qlen, rlen = qe - qb, re - rb
    w2 = first_w2(scoring, opt_w, qlen, rlen, truesc, reg_w)
    band = band_of(scoring, qlen, rlen, w2)
    if band is None:
        return (0, 0, 0, "trivial")
    w, n_col = band
    kind = next((k for k, cols in KIND_COLS if n_col <= cols), "slow")
    return (w2, w, n_col, kind)


def is_long(qlen, rlen):
    return qlen > CG_LDS_MAX or rlen > CG_LDS_MAX


def slow_form(qlen, rlen):
    """the cigar_kernel instantiation that takes a job of the slow list"""
    if is_long(qlen, rlen):
        return "long"
    need = (qlen + 63) >> 6
    return next(name for c, name in SLOW_FORMS if need <= c)


def retry_trace(scoring, opt_w, qlen, rlen, truesc, reg_w, score_of):
    """the loop of mem_reg2aln.  score_of(w2) -> the global score of a round -> ([(w2, score), ...], how the loop ended: "reached" (the score came within a of
    truesc), "repeat" (the score of the round before), "cap" (the band is 4 opt_w), "rounds" (three rounds))"""
    a = scoring[0]
    w2 = first_w2(scoring, opt_w, qlen, rlen, truesc, reg_w)
    rounds, last, it = [], -(1 << 30), 0
    while True:
        w2 = min(w2, opt_w << 2)
        sc = score_of(w2)
        rounds.append((w2, sc))
        if sc == last:
            return rounds, "repeat"
        if w2 == opt_w << 2:
            return rounds, "cap"
        last = sc
        w2 <<= 1
        it += 1
        if it >= 3:
            return rounds, "rounds" if sc < truesc - a else "reached"
        if sc >= truesc - a:
            return rounds, "reached"


def class_counts(jobs, scoring, opt_w):
    """what the [cigar] line of BMH_CIGAR_STATS prints for a batch: the lists as cigar_classify_kernel leaves them (F2, F3, F5, F10, F16, slow)"""
    kinds = [route(scoring, opt_w, j.qb, j.qe, j.rb, j.re, j.truesc, j.reg_w)[3] for j in jobs]
    return tuple(kinds.count(k) for k in ("F2", "F3", "F5", "F10", "F16", "slow"))


def finish_windows(ops_dp, qlen, rlen, w):
    """cigar_finish_kernel's walk through windows of 16 x 16 cells, replayed on the operations of the DP (in DP order, before the squeeze): the set of
    (state, event): state "E" (deletion) or "F" (insertion); "enter_first" / "enter_last": the gap's first step of the walk is the first / the last step of a
    window; "leave_last": its last step is the last of a window (the H step after it opens the next); "inside": a window ends inside the gap; "corner": a gap
    step in a window that reaches above row 0 or left of column 0 (the clamped corner)"""
    steps = []
    for c in ops_dp[::-1]:
        steps += [int(c & 0xf)] * int(c >> 4)
    i, k = rlen - 1, min(rlen + w, qlen) - 1
    ev, s = set(), 0
    while i >= 0 and k >= 0 and s < len(steps):
        i0, k0 = i, k
        first = True
        while i >= 0 and k >= 0 and i0 - i < 16 and k0 - k < 16 and s < len(steps):
            op = steps[s]
            di, dk = int(op != 1), int(op != 2)
            last = i0 - (i - di) >= 16 or k0 - (k - dk) >= 16
            if op:
                st = "E" if op == 2 else "F"
                enters = s == 0 or steps[s - 1] != op
                leaves = s + 1 == len(steps) or steps[s + 1] != op
                if enters and first: ev.add((st, "enter_first"))
                if enters and last: ev.add((st, "enter_last"))
                if leaves and last: ev.add((st, "leave_last"))
                if last and not leaves: ev.add((st, "inside"))
                if i0 < 15 or k0 < 15: ev.add((st, "corner"))
            i -= di; k -= dk; s += 1; first = False
    return ev


# ---------------------------------------------------------------------------------------------------------------- the table

class Table:
    def __init__(self):
        self.batches = {}

    def batch(self, name, family, scoring=DEFAULT, opt_w=100, stride=8, max_cigar=None, md_cap=None):
        assert name not in self.batches and family in FAMILIES
        b = SimpleNamespace(name=name, family=family, scoring=tuple(scoring), opt_w=opt_w, stride=stride, max_cigar=max_cigar, md_cap=md_cap, jobs=[])
        self.batches[name] = b
        return b


def _apply(T, edits, rng):
    """Q for the target T: edits = (position in T, op, n), op "X" a substitution, "N" an N, "D" T[p:p+n] missing from Q, "I" n bases in front of T[p] (one base,
    repeated, that continues neither side) -> (Q, the number of matches, substitutions, Ns, deletions [n], insertions [n])"""
    out, at = [], 0
    n_x = n_n = 0
    dels, inss = [], []
    for p, op, n in sorted(edits, key=lambda e: (e[0], e[1] != "I")):
        assert p >= at, "edits overlap"
        out.append(T[at:p]); at = p
        if op == "I":
            z = min(set(range(4)) - {int(T[p - 1]) if p else -1, int(T[p]) if p < len(T) else -1})
            out.append(np.full(n, z, np.uint8)); inss.append(n)
        elif op == "D":
            at = p + n; dels.append(n)
        elif op == "X":
            out.append(np.array([(int(T[p]) + 1 + p % 3) & 3], np.uint8)); at = p + 1; n_x += 1
        else:
            out.append(np.array([4], np.uint8)); at = p + 1; n_n += 1
    out.append(T[at:])
    Q = np.ascontiguousarray(np.concatenate(out), dtype=np.uint8)
    return Q, len(T) - sum(dels) - n_x - n_n, n_x, n_n, dels, inss


def add(b, name, rlen, edits=(), flip=False, clips=(0, 0), truesc=None, dsc=0, reg_w=None, at=None, exact=False, expect=None, limits=(), **extra):
    """one job, written in DP coordinates.  at: where the region starts on the forward genome (default: drawn from the name); flip: the region lies on the
    reverse half of the text, DP coordinates run against it.  truesc: the local score (default: what the edits cost, plus dsc)."""
    name = f"{name}/{'r' if flip else 'f'}"
    rng = np.random.default_rng(zlib.crc32(f"{b.name}:{name}".encode()))
    if at is None:
        at = 100 + int(rng.integers(0, L_PAC - rlen - 200))
        if at < DINUC + 100 and at + rlen > HOMOPOLYMER - 100:
            at = DINUC + 200
    while True:
        assert 0 <= at and at + rlen <= L_PAC
        rb = 2 * L_PAC - (at + rlen) if flip else at
        re = rb + rlen
        S = TEXT[rb:re]
        T = S[::-1] if flip else S
        # exact: no deletion has a placement of the same cost further left (the base in front of it is not its last one)
        if not exact or all(op != "D" or p == 0 or T[p - 1] != T[p + n - 1] for p, op, n in edits):
            break
        at += 1
    Q, n_match, n_x, n_n, dels, inss = _apply(T, edits, rng)
    a, bb, od, ed, oi, ei = b.scoring
    honest = a * n_match - bb * n_x - n_n - sum(od + ed * n for n in dels) - sum(oi + ei * n for n in inss)
    part = Q[::-1] if flip else Q
    c5, c3 = clips
    read = to_ascii(np.concatenate([rng.integers(0, 4, size=c5).astype(np.uint8), part, rng.integers(0, 4, size=c3).astype(np.uint8)]))
    j = SimpleNamespace(name=name, batch=b.name, read=read, qb=c5, qe=c5 + len(Q), rb=rb, re=re, truesc=honest + dsc if truesc is None else truesc,
                        reg_w=b.opt_w if reg_w is None else reg_w, flip=flip, limits=tuple(limits), extra=dict(extra))
    return _finish(b, j, expect)


def add_raw(b, name, read, qb, qe, rb, re, truesc, expect, limits=(), **extra):
    """a job given as it stands (the regions the reference rejects)"""
    j = SimpleNamespace(name=name, batch=b.name, read=bytes(read), qb=qb, qe=qe, rb=rb, re=re, truesc=truesc, reg_w=b.opt_w, flip=rb >= L_PAC, limits=tuple(limits),
                        extra=dict(extra))
    return _finish(b, j, expect)


_RECORD = object()


def _finish(b, j, expect):
    assert b.stride == 16 or j.reg_w == b.opt_w, "a band of its own needs the records of 16 words"
    j.route = route(b.scoring, b.opt_w, j.qb, j.qe, j.rb, j.re, j.truesc, j.reg_w)
    assert expect is not None and (expect is _RECORD or j.route == tuple(expect)), (b.name, j.name, j.route, expect)
    assert all(x.name != j.name for x in b.jobs), j.name
    assert 0 <= j.rb and j.re <= 2 * L_PAC and 0 <= j.qb and j.qe <= len(j.read)
    b.jobs.append(j)
    return j


def both(b, name, rlen, **kw):
    return [add(b, name, rlen, flip=f, **kw) for f in (False, True)]


def _kind_of(n_col):
    return next((k for k, cols in KIND_COLS if n_col <= cols), "slow")


def _kinds(t):
    b = t.batch("kinds", "kinds")
    # n_col through a gap's length: one gap of d bases asks for w = d + 3, n_col = 2 d + 7
    for d, n_col, kind in ((12, 31, "F2"), (13, 33, "F3"), (20, 47, "F3"), (21, 49, "F5"), (36, 79, "F5"), (37, 81, "F10"), (76, 159, "F10"), (77, 161, "F16"),
                           (124, 255, "F16"), (125, 257, "slow")):
        both(b, f"del{d}", 300 + d, edits=[(150, "D", d)], expect=(min(d + 2, 100), d + 3, n_col, kind), limits=[f"gap_ncol{n_col}", f"del_ncol{n_col}"])
        both(b, f"ins{d}", 300 - d, edits=[(140, "I", d)], expect=(min(d + 2, 100), d + 3, n_col, kind), limits=[f"gap_ncol{n_col}", f"ins_ncol{n_col}"])
    # n_col = qlen under a band wider than the query: a deletion of d bases with 2 (d + 3) + 1 > qlen
    for q, kind in ((32, "F2"), (33, "F3"), (48, "F3"), (49, "F5"), (80, "F5"), (81, "F10"), (160, "F10"), (161, "F16"), (256, "F16"), (257, "slow")):
        d = (q + 1) // 2 - 2
        assert 2 * (d + 3) + 1 > q
        both(b, f"qlen{q}", q + d, edits=[(q // 2, "D", d)], expect=(min(d + 2, 100), d + 3, q, kind), limits=[f"qlen_ncol{q}"])
    # the gate of the one-run jobs: qlen a - truesc on both sides of 2 (o + e - a) = 12
    both(b, "gate11", 100, edits=[(30, "X", 1), (70, "X", 1)], truesc=89, expect=(0, 0, 0, "trivial"), limits=["gate_below"])
    both(b, "gate12", 100, edits=[(30, "X", 1), (70, "X", 1)], truesc=88, expect=(8, 8, 17, "F2"), limits=["gate_at"])
    # a one-run job whose true score is far below truesc: the loop runs it twice and leaves it one M run
    both(b, "one_run_low", 120, edits=[(3, "X", 1), (40, "N", 1), (41, "X", 1), (77, "X", 1), (100, "N", 1), (119, "X", 1)], truesc=120, expect=(0, 0, 0, "trivial"),
         limits=["one_run_low"])


def _two_gaps(n=20):
    """a deletion and an insertion of n bases 100 apart: the path leaves the diagonal by n, whatever the lengths say"""
    return [(50, "D", n), (170, "I", n)]


def _retry(t):
    b = t.batch("retry", "retry")
    # three substitutions in 120 bases: the global score is 105 under every band
    both(b, "at_truesc_minus_a", 120, edits=[(30, "X", 1), (60, "X", 1), (90, "X", 1)], truesc=106, expect=(10, 10, 21, "F2"), limits=["score_at"], exit="reached", rounds=1)
    both(b, "below_truesc_minus_a", 120, edits=[(30, "X", 1), (60, "X", 1), (90, "X", 1)], truesc=107, expect=(9, 9, 19, "F2"), limits=["score_below", "exit_repeat"],
         exit="repeat", rounds=2)
    # bands of 8, 16 and 32 for two gaps of 20: three rounds
    both(b, "three_rounds", 220, edits=_two_gaps(), truesc=208, expect=(8, 8, 17, "F2"), limits=["exit_rounds"], exit="rounds", rounds=3)
    # demoted jobs at both sides of every wave-per-region instantiation
    for q in (64, 65, 128, 129, 192, 193, 320, 321, 512, 513, 704, 705):
        both(b, f"demoted{q}", q, edits=[(q // 4, "X", 1), (q // 2, "X", 1), (3 * q // 4, "X", 1)], dsc=2, expect=(9, 9, 19, "F2"), limits=[f"demoted_qlen{q}"],
             exit="repeat", rounds=2)
    b = t.batch("retry_w4", "retry", opt_w=4)
    both(b, "cap_third_round", 220, edits=_two_gaps(), truesc=208, expect=(4, 4, 9, "F2"), limits=["exit_cap"], exit="cap", rounds=3)
    b = t.batch("retry_w4_s16", "retry", opt_w=4, stride=16)
    both(b, "cap_second_round", 220, edits=_two_gaps(), truesc=208, reg_w=8, expect=(8, 8, 17, "F2"), limits=["exit_cap", "reg_w_above_opt_w"], exit="cap", rounds=2)
    both(b, "first_w2_is_cap", 220, edits=_two_gaps(), truesc=200, reg_w=16, expect=(16, 16, 33, "F3"), limits=["first_w2_cap"], exit="cap", rounds=1)
    both(b, "first_w2_is_cap_w100", 220, edits=_two_gaps(), truesc=200, reg_w=100, expect=(16, 16, 33, "F3"), limits=["first_w2_cap"], exit="cap", rounds=1)
    b = t.batch("retry_s16", "retry", stride=16)
    both(b, "del125_w300", 425, edits=[(150, "D", 125)], reg_w=300, expect=(127, 128, 257, "slow"), limits=["reg_w_above_opt_w"])
    both(b, "del125_w110", 425, edits=[(150, "D", 125)], reg_w=110, expect=(110, 128, 257, "slow"), limits=["reg_w_above_opt_w"])
    both(b, "wide_w120", 300, edits=[(50, "X", 1), (150, "X", 1), (250, "X", 1)], truesc=146, reg_w=120, expect=(120, 73, 147, "F10"), limits=["reg_w_above_opt_w"])
    both(b, "del12_w100", 312, edits=[(150, "D", 12)], reg_w=100, expect=(14, 15, 31, "F2"))


def _trace(t):
    b = t.batch("trace", "trace")
    # a gap of five bases whose distance from the alignment's end sweeps over the edge of the first window (and, one window on, of the second)
    for dist in range(9, 19):
        both(b, f"del5_end{dist}", 96, edits=[(96 - 5 - dist, "D", 5)], exact=True, expect=(7, 8, 17, "F2"), limits=["window_sweep"])
        both(b, f"ins5_end{dist}", 91, edits=[(91 - dist, "I", 5)], expect=(7, 8, 17, "F2"), limits=["window_sweep"])
    for dist in (27, 32):
        both(b, f"del20_end{dist}", 116, edits=[(116 - 20 - dist, "D", 20)], exact=True, expect=(22, 23, 47, "F3"), limits=["window_sweep"])
        both(b, f"ins20_end{dist}", 96, edits=[(96 - dist, "I", 20)], expect=(22, 23, 47, "F3"), limits=["window_sweep"])
    # gaps in the first rows and columns: the window's clamped corner
    for rlen in (83, 75):
        both(b, f"del3_row5_of{rlen}", rlen, edits=[(5, "D", 3)], expect=(5, 6, 13, "F2"), limits=["corner"])
    for rlen in (80, 76):
        both(b, f"ins3_col6_of{rlen}", rlen, edits=[(6, "I", 3)], expect=(5, 6, 13, "F2"), limits=["corner"])
    # rows / columns left over after the walk; a leading and a trailing deletion are squeezed out
    both(b, "lead_del6", 86, edits=[(0, "D", 6)], truesc=80, expect=(6, 9, 19, "F2"), limits=["rows_left", "lead_del"])
    both(b, "trail_del6", 86, edits=[(80, "D", 6)], truesc=80, exact=True, expect=(6, 9, 19, "F2"), limits=["trail_del"])
    both(b, "lead_ins4", 80, edits=[(0, "I", 4)], truesc=80, expect=(4, 7, 15, "F2"), limits=["cols_left"])
    both(b, "trail_ins4", 80, edits=[(80, "I", 4)], truesc=80, expect=(4, 7, 15, "F2"), limits=["trail_ins"])
    # placements of equal cost: two of eight As, one of five ACs -- the left-most one on the forward genome, on either strand
    for nm, p0, ed in (("homo_del2", HOMOPOLYMER - 40, (43, "D", 2)), ("dinuc_del2", DINUC - 40, (44, "D", 2))):
        both(b, nm, 90, edits=[ed], at=p0, expect=(4, 5, 11, "F2"), limits=["equal_cost"])
    # soft clips on one and on both sides, with a gap and a substitution
    for nm, clips in (("clip5", (7, 0)), ("clip3", (0, 9)), ("clip_both", (11, 5))):
        both(b, nm + "_del4", 104, edits=[(20, "X", 1), (50, "D", 4)], clips=clips, exact=True, expect=(11, 11, 23, "F2"), limits=[nm])
        both(b, nm + "_one_run", 100, edits=[(20, "X", 1)], clips=clips, expect=(0, 0, 0, "trivial"), limits=[nm])
    # N in the read: in a run, beside a gap, at both ends
    both(b, "n_del4", 104, edits=[(0, "N", 1), (49, "N", 1), (50, "D", 4), (54, "N", 1), (103, "N", 1)], expect=(14, 14, 29, "F2"), limits=["n_bases"])
    both(b, "n_one_run", 100, edits=[(0, "N", 1), (50, "N", 1), (99, "N", 1)], expect=(0, 0, 0, "trivial"), limits=["n_bases"])
    # MD numbers of one, two and three digits (four: the long batch)
    both(b, "md_digits", 300, edits=[(5, "X", 1), (53, "X", 1), (184, "X", 1)], expect=(11, 11, 23, "F2"), limits=["md_digits_123"])
    both(b, "md_digits_one_run", 300, edits=[(5, "X", 1), (53, "X", 1), (184, "X", 1)], truesc=300, expect=(0, 0, 0, "trivial"), limits=["md_digits_123"])
    # a substitution at the first and at the last base
    both(b, "mm_first_last", 100, edits=[(0, "X", 1), (99, "X", 1)], truesc=88, expect=(8, 8, 17, "F2"), limits=["mm_first_last"])
    both(b, "mm_first_last_one_run", 100, edits=[(0, "X", 1), (99, "X", 1)], expect=(0, 0, 0, "trivial"), limits=["mm_first_last"])
    # substitutions on the chunk edges of the NM / MD loops: 16 bases a step in cigar_finish_kernel, 64 in cigar_kernel
    edge = [(p, "X", 1) for p in (15, 16, 63, 64, 127, 128)]
    both(b, "mm_chunk_edges", 200, edits=edge, expect=(26, 26, 53, "F5"), limits=["mm_chunk_edges"])
    both(b, "mm_chunk_edges_one_run", 200, edits=edge, truesc=189, expect=(0, 0, 0, "trivial"), limits=["mm_chunk_edges"])
    both(b, "mm_chunk_edges_after_gap", 203, edits=[(10, "D", 3)] + [(13 + p, "X", 1) for p in (15, 16, 63, 64, 127, 128)], expect=(35, 35, 71, "F5"), limits=["mm_chunk_edges"])


def _geometry(t):
    b = t.batch("geometry", "geometry")
    # the four ends of the text: rb = 0 and re = l_pac on the forward half, rb = l_pac and re = 2 l_pac on the reverse half
    add(b, "rb_0", 104, edits=[(0, "X", 1), (50, "D", 4)], at=0, expect=(11, 11, 23, "F2"), limits=["rb_0"])
    add(b, "re_l_pac", 104, edits=[(50, "D", 4), (103, "X", 1)], at=L_PAC - 104, expect=(11, 11, 23, "F2"), limits=["re_l_pac"])
    add(b, "rb_l_pac", 104, edits=[(50, "D", 4), (103, "X", 1)], at=L_PAC - 104, flip=True, expect=(11, 11, 23, "F2"), limits=["rb_l_pac"])
    add(b, "re_2l_pac", 104, edits=[(0, "X", 1), (50, "D", 4)], at=0, flip=True, expect=(11, 11, 23, "F2"), limits=["re_2l_pac"])
    add(b, "rb_0_one_run", 100, at=0, expect=(0, 0, 0, "trivial"), limits=["rb_0"])
    add(b, "re_2l_pac_one_run", 100, at=0, flip=True, expect=(0, 0, 0, "trivial"), limits=["re_2l_pac"])
    assert [(j.rb, j.re) for j in b.jobs[:4]] == [(0, 104), (L_PAC - 104, L_PAC), (L_PAC, L_PAC + 104), (2 * L_PAC - 104, 2 * L_PAC)]
    # what bwa_gen_cigar2 rejects: flag 2 (the reference has no CIGAR for these: they are not in the fixture)
    read = to_ascii(TEXT[L_PAC - 50:L_PAC + 50])
    rej = (0, 0, 0, "reject")
    add_raw(b, "bridging", read, 0, 100, L_PAC - 50, L_PAC + 50, 100, rej, limits=["bridging"])
    add_raw(b, "bridging_by_one", read, 0, 100, L_PAC - 99, L_PAC + 1, 100, rej, limits=["bridging"])
    add_raw(b, "empty_region", read, 0, 100, 500, 500, 100, rej, limits=["empty"])
    add_raw(b, "inverted_region", read, 0, 100, 600, 500, 100, rej, limits=["inverted"])
    add_raw(b, "empty_query", read, 40, 40, 500, 600, 100, rej, limits=["empty"])
    add_raw(b, "inverted_query", read, 60, 40, 500, 600, 100, rej, limits=["inverted"])
    # sides of CG_LDS_MAX and one more.  A narrow band: the fast path takes them whatever their length
    for q in (704, 705):
        both(b, f"narrow_qlen{q}", q, edits=[(q // 4, "X", 1), (q // 2, "X", 1), (3 * q // 4, "X", 1)], expect=(11, 11, 23, "F2"), limits=[f"narrow_side{q}"])
        both(b, f"narrow_rlen{q}", q, edits=[(300, "D", q - 600)], expect=(100, q - 597, 2 * (q - 597) + 1, "F16"), limits=[f"narrow_side{q}"])
    # a wide band: the last LDS form at 704, the long form at 705
    for q in (704, 705):
        both(b, f"wide_qlen{q}", q - 125, edits=[(300, "I", 125)], expect=(100, 128, 257, "slow"), limits=[f"wide_qlen{q}"], form="11,8" if q == 704 else "long")
        both(b, f"wide_rlen{q}", q, edits=[(300, "D", 125)], expect=(100, 128, 257, "slow"), limits=[f"wide_rlen{q}"], form="11,8" if q == 704 else "long")
    b = t.batch("long", "geometry")
    both(b, "del130_md4", 1330, edits=[(40, "X", 1), (1141, "D", 130)], expect=(100, 133, 267, "slow"), limits=["long_form", "md_digits_4"], form="long")
    add(b, "ins126", 1374, edits=[(700, "I", 126), (1300, "X", 1)], expect=(100, 129, 259, "slow"), limits=["long_form"], form="long")
    both(b, "one_run_md4", 1200, edits=[(1150, "X", 1)], expect=(0, 0, 0, "trivial"), limits=["md_digits_4"])
    both(b, "narrow_1000", 1000, edits=[(250, "X", 1), (500, "X", 1), (750, "X", 1)], expect=(11, 11, 23, "F2"), limits=["long_fast"])
    add_raw(b, "bridging_long", to_ascii(TEXT[L_PAC - 400:L_PAC - 100]), 0, 300, L_PAC - 400, L_PAC + 400, 300, (0, 0, 0, "reject"), limits=["bridging"])
    # a long-form job whose |rlen - qlen| + 3 exceeds 4 opt_w
    b = t.batch("long_w20", "geometry", opt_w=20)
    both(b, "del130", 850, edits=[(400, "D", 130)], expect=(20, 133, 267, "slow"), limits=["long_beyond_4w"], form="long")
    assert all(abs((j.re - j.rb) - (j.qe - j.qb)) + 3 > 4 * b.opt_w for j in b.jobs)
    both(b, "del12", 312, edits=[(150, "D", 12)], expect=(14, 15, 31, "F2"))


def _gaps14(n_seg):
    """a leading insertion of four bases and a gap of one base between every two of n_seg segments of 14 bases (insertions, the last one a deletion): 2 n_seg
    operations"""
    ed = [(0, "I", 4)] + [(14 * s, "I", 1) for s in range(1, n_seg - 1)] + [(14 * (n_seg - 1), "D", 1)]
    return 14 * n_seg + 1, ed


def _slots(t):
    """max_cigar 16: the walk keeps max_cigar - 2 = 14 operations; md_cap 24: an MD string of 23 characters and its NUL"""
    b = t.batch("slots", "slots", max_cigar=16, md_cap=24)
    mm7 = [(10 + 11 * k, "X", 1) for k in range(7)]
    r14, e14 = _gaps14(7)
    r16, e16 = _gaps14(8)
    r12, e12 = _gaps14(6)
    for flip in (False, True):
        add(b, "ops12_two_clips", r12, edits=e12, clips=(3, 4), flip=flip, expect=(42, 24, 49, "F5"), small=0, ops=12)
        add(b, "ops14_two_clips", r14, edits=e14, clips=(3, 4), flip=flip, expect=(49, 29, 59, "F5"), limits=["ops_fit"], small=0, ops=14)
        add(b, "ops16_two_clips", r16, edits=e16, clips=(3, 4), flip=flip, expect=(56, 33, 67, "F5"), limits=["ops_over"], small=1, ops=16)
        add(b, "md23", 87, edits=mm7, flip=flip, expect=(31, 20, 41, "F3"), limits=["md_fit"], small=0, md_len=23)
        add(b, "ops15_no_clips", r14 + 5, edits=e14 + [(r14 + 5, "I", 2)], flip=flip, expect=(57, 31, 63, "F5"), limits=["ops_over"], small=1, ops=15)
        add(b, "md24", 177, edits=mm7, flip=flip, expect=(31, 31, 63, "F5"), limits=["md_over"], small=8, md_len=24)
        add(b, "md23_one_run", 87, edits=mm7, truesc=87, flip=flip, expect=(0, 0, 0, "trivial"), limits=["md_fit"], small=0, md_len=23)
        add(b, "md24_one_run", 177, edits=mm7, truesc=177, flip=flip, expect=(0, 0, 0, "trivial"), limits=["md_over"], small=8, md_len=24)
        add(b, "ops14_one_clip", r14, edits=e14, clips=(0, 6), flip=flip, expect=(49, 29, 59, "F5"), limits=["ops_fit"], small=0, ops=14)


# (w2, w, n_col, kind) of the jobs of _scoring_batch under every scoring, in order: recorded from route() when the batch was written, and held here
SCORING_ROUTES = {
    "default": ((0, 0, 0, 'trivial'), (8, 8, 17, 'F2'), (10, 10, 21, 'F2'), (9, 9, 19, 'F2'), (22, 22, 45, 'F3'), (20, 20, 41, 'F3'), (23, 24, 49, 'F5'), (6, 9, 19, 'F2'), (8, 8, 17, 'F2'), (7, 8, 17, 'F2'), (7, 8, 17, 'F2')),
    "scaled2": ((0, 0, 0, 'trivial'), (8, 8, 17, 'F2'), (10, 10, 21, 'F2'), (9, 9, 19, 'F2'), (21, 21, 43, 'F3'), (20, 20, 41, 'F3'), (23, 24, 49, 'F5'), (6, 9, 19, 'F2'), (8, 8, 17, 'F2'), (7, 8, 17, 'F2'), (7, 8, 17, 'F2')),
    "ins_dear": ((0, 0, 0, 'trivial'), (8, 8, 17, 'F2'), (10, 10, 21, 'F2'), (9, 9, 19, 'F2'), (22, 22, 45, 'F3'), (49, 42, 85, 'F10'), (23, 24, 49, 'F5'), (6, 9, 19, 'F2'), (8, 8, 17, 'F2'), (7, 8, 17, 'F2'), (20, 20, 41, 'F3')),
    "del_dear": ((0, 0, 0, 'trivial'), (8, 8, 17, 'F2'), (10, 10, 21, 'F2'), (9, 9, 19, 'F2'), (51, 42, 85, 'F10'), (20, 20, 41, 'F3'), (68, 46, 93, 'F10'), (6, 9, 19, 'F2'), (8, 8, 17, 'F2'), (20, 20, 41, 'F3'), (7, 8, 17, 'F2')),
    "lut_edge": ((0, 0, 0, 'trivial'), (5, 5, 11, 'F2'), (32, 29, 59, 'F5'), (31, 29, 59, 'F5'), (27, 27, 55, 'F5'), (26, 26, 53, 'F5'), (23, 24, 49, 'F5'), (6, 9, 19, 'F2'), (5, 5, 11, 'F2'), (7, 8, 17, 'F2'), (7, 8, 17, 'F2')),
    "generic": ((0, 0, 0, 'trivial'), (1, 3, 7, 'F2'), (21, 21, 43, 'F3'), (21, 21, 43, 'F3'), (30, 30, 61, 'F5'), (25, 25, 51, 'F5'), (23, 24, 49, 'F5'), (6, 9, 19, 'F2'), (1, 3, 7, 'F2'), (7, 8, 17, 'F2'), (7, 8, 17, 'F2')),
    "b0": ((0, 0, 0, 'trivial'), (8, 8, 17, 'F2'), (0, 0, 0, 'trivial'), (0, 0, 0, 'trivial'), (18, 18, 37, 'F3'), (16, 16, 33, 'F3'), (23, 24, 49, 'F5'), (6, 9, 19, 'F2'), (8, 8, 17, 'F2'), (7, 8, 17, 'F2'), (7, 8, 17, 'F2')),
    "free_open": ((0, 0, 0, 'trivial'), (2, 3, 7, 'F2'), (16, 16, 33, 'F3'), (15, 15, 31, 'F2'), (22, 22, 45, 'F3'), (20, 20, 41, 'F3'), (23, 24, 49, 'F5'), (6, 9, 19, 'F2'), (2, 3, 7, 'F2'), (7, 8, 17, 'F2'), (7, 8, 17, 'F2')),
}


def _scoring_batch(t, sname):
    sc = SCORINGS[sname]
    a, bb, od, ed, oi, ei = sc
    b = t.batch("sc_" + sname, "scorings", scoring=sc)
    gate = min((od + ed - a) << 1, (oi + ei - a) << 1)
    specs = [
        ("gate_below", 100, dict(edits=[(30, "X", 1)], truesc=100 * a - gate + 1)),
        ("gate_at", 100, dict(edits=[(30, "X", 1)], truesc=100 * a - gate)),
        ("score_at", 120, dict(edits=[(30, "X", 1), (60, "X", 1), (90, "X", 1)], dsc=a)),
        ("score_below", 120, dict(edits=[(30, "X", 1), (60, "X", 1), (90, "X", 1)], dsc=a + 1)),
        ("del13", 163, dict(edits=[(20, "X", 1), (80, "D", 13), (140, "N", 1)], clips=(5, 0))),
        ("ins13", 137, dict(edits=[(20, "X", 1), (70, "I", 13)], clips=(0, 6))),
        ("del21", 171, dict(edits=[(75, "D", 21)])),
        ("lead_del6", 86, dict(edits=[(0, "D", 6)], truesc=80 * a)),
        ("two_gaps", 220, dict(edits=_two_gaps(), truesc=220 * a - gate)),
        ("del5_end15", 96, dict(edits=[(96 - 5 - 15, "D", 5)])),
        ("ins5_end16", 91, dict(edits=[(91 - 16, "I", 5)])),
    ]
    want = SCORING_ROUTES.get(sname)                               # (None only while the routes of a new scoring are being recorded: table() refuses it)
    k = 0
    for flip in (False, True):
        for nm, rlen, kw in specs:
            add(b, nm, rlen, flip=flip, expect=want[k % len(specs)] if want else _RECORD, limits=["sc_" + nm], **kw)
            k += 1
    return b


@functools.lru_cache(maxsize=1)
def table():
    assert set(SCORING_ROUTES) == set(SCORINGS)
    return _build()


def _build():
    t = Table()
    _kinds(t); _retry(t); _trace(t); _geometry(t); _slots(t)
    for sname in SCORINGS:
        _scoring_batch(t, sname)
    for b in t.batches.values():
        b.n = len(b.jobs)
        lens = np.array([len(j.read) for j in b.jobs], np.int64)
        b.reads = np.frombuffer(b"".join(j.read for j in b.jobs), np.uint8).copy()
        b.lens = lens.astype(np.uint32)
        b.offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint32)
        for k, j in enumerate(b.jobs):
            j.read_id, j.index = k, k
    return t


def batches():
    return table().batches


def batch_names():
    return tuple(batches())


def all_jobs():
    """every job in table order"""
    return [j for b in batches().values() for j in b.jobs]


def fixture_jobs():
    """the jobs the reference has an answer for, in table order: all but the rejected ones"""
    return [j for j in all_jobs() if j.route[3] != "reject"]


def key_of(j):
    return f"{j.batch}:{j.name}"


def regs_of(b, jobs=None, stride=None, read_of=None):
    """the region records as bmh_cigar_batch takes them: int32 [n][stride] = {read, score, qb, qe, rb_lo, rb_hi, re_lo, re_hi} (+ {truesc, w, ...} when stride is
    16; the score word of such a record is not the one the kernels may use: it holds a number no job has)"""
    jobs = b.jobs if jobs is None else jobs
    stride = b.stride if stride is None else stride
    out = np.zeros((len(jobs), stride), np.int32)
    for k, j in enumerate(jobs):
        rd = j.read_id if read_of is None else read_of[k]
        out[k, :8] = [rd, j.truesc if stride == 8 else 7, j.qb, j.qe, j.rb & 0xFFFFFFFF, j.rb >> 32, j.re & 0xFFFFFFFF, j.re >> 32]
        if stride == 16:
            out[k, 8], out[k, 9] = j.truesc, j.reg_w
        else:
            assert j.reg_w == b.opt_w
    return out


def digest():
    """of everything a result depends on: the genome, and scoring, band, reads and regions of every job in table order"""
    h = hashlib.sha256()
    h.update(GENOME.tobytes())
    for b in batches().values():
        h.update(b.name.encode()); h.update(np.array([*b.scoring, b.opt_w, b.stride, b.max_cigar or 0, b.md_cap or 0], np.int64).tobytes())
        for j in b.jobs:
            h.update(j.name.encode()); h.update(j.read)
            h.update(np.array([j.qb, j.qe, j.rb, j.re, j.truesc, j.reg_w], np.int64).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------- the reference's answer

def batch_of(j):
    return batches()[j.batch]


def reference_row(ref_tail, j):
    """oracle_py.RefTail.reg2aln, the reference's mem_reg2aln, on one job -> dict(pos, is_rev, cigar, NM, MD)"""
    b = batch_of(j)
    return ref_tail.reg2aln(b.scoring, b.opt_w, L_PAC, PAC, j.read, j.qb, j.qe, j.rb, j.re, j.truesc, j.reg_w)


def pack_rows(rows):
    """rows of dict(pos, is_rev, cigar, NM, MD) -> the arrays of the fixture"""
    aln = np.array([[r["pos"], r["is_rev"], len(r["cigar"]), r["NM"]] for r in rows], np.int64)
    cg_off = np.concatenate([[0], np.cumsum([len(r["cigar"]) for r in rows])]).astype(np.int64)
    md_off = np.concatenate([[0], np.cumsum([len(r["MD"]) for r in rows])]).astype(np.int64)
    cigar = np.concatenate([np.asarray(r["cigar"], np.uint32) for r in rows]).astype(np.uint32)
    md = np.frombuffer("".join(r["MD"] for r in rows).encode(), np.uint8).copy()
    return dict(aln=aln, cigar=cigar, cg_off=cg_off, md=md, md_off=md_off)


def unpack_rows(z):
    """the fixture's arrays -> key_of(job) -> dict(pos, is_rev, cigar, NM, MD), for fixture_jobs() in table order"""
    jobs = fixture_jobs()
    aln, cigar, cg_off, md, md_off = (np.asarray(z[k]) for k in ("aln", "cigar", "cg_off", "md", "md_off"))
    assert aln.shape == (len(jobs), 4) and len(cg_off) == len(md_off) == len(jobs) + 1
    out = {}
    for k, j in enumerate(jobs):
        cg = cigar[cg_off[k]:cg_off[k + 1]].astype(np.uint32)
        assert len(cg) == aln[k, 2]
        out[key_of(j)] = dict(pos=int(aln[k, 0]), is_rev=int(aln[k, 1]), cigar=cg, NM=int(aln[k, 3]), MD=md[md_off[k]:md_off[k + 1]].tobytes().decode())
    return out


def same_row(x, y):
    return (x["pos"], x["is_rev"], x["NM"], x["MD"]) == (y["pos"], y["is_rev"], y["NM"], y["MD"]) and np.array_equal(x["cigar"], y["cigar"])


def dp_ops(j, row):
    """the operations of a row without its clips (the operations of the DP, but for a squeezed deletion)"""
    return row["cigar"][(row["cigar"] & 0xf) != 3]
