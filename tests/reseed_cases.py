"""Hand-made read batches for the re-seeding kernels (csrc/reseed_kernels.hip against the reference's mem_collect_intv with re_seed: bwt_smem1 with a
min_intv, bwt_seed_strategy1, ks_introsort(mem_intv)): every structural limit of the selection, of round 2's forward list, its overflow into the second
launch and its backward rounds, of round 3 and of the merge, each reached on purpose.  Plain numpy plus the oracle's rank function, no tests, no GPU.

The genomes, Batch and make_case are those of tests/seed_cases.py (world("main"): the staircase gives round-2 forward lists of any chosen length, the
planted 40-mers both sides of split_width and max_mem_intv; world("small"): the A-run).  One genome is added, world("long"): 60 kb of random bases, for a
read whose seeds begin and end beyond 32 767.

A case is one batch plus min_seed_len and the three re-seeding options, and `must`: name -> bool, what the case is about.  Every predicate is evaluated
when the case is built, on a restatement in Python (restate_read) of the reference's three rounds over the oracle's rank function: mem_collect_intv
(src/bwamem.c:266-297), bwt_smem1a with a min_intv (src/bwt.c:483-556), bwt_seed_strategy1 (src/bwt.c:568-590).  It returns the groups and what the
predicates need: per task x, min_intv, the forward list's length, how the forward walk ended, the backward rounds and how they ended, rank steps, entries
dropped for an equal size, hits dropped as contained, hits shorter than min_seed_len; per read the round-3 seeds and whether an empty interval was carried.
restate() adds what bmh_reseed_last_counts must report for the case: tasks, tasks whose list does not fit the first launch's column, groups per round, and
(device_steps) the rank steps of rounds 2 and 3, at any column size.

Cost is a condition of the table, a `must` of every case: a lane of the device walks its task alone, so no task walks more than 100 000 rank steps and no
case more than 2 million.  The 65 535-base poly-A read of seed_cases stays out of it under re-seeding: about 5e8 sequential steps in one lane."""
from __future__ import annotations

import ctypes as C
import functools
import hashlib
import os
from types import SimpleNamespace

import numpy as np

import seed_cases
from seed_cases import M64, MER_COUNTS, PLAIN_AT, SEED_KEYS, Batch, mer_read, sa_of, sub, world

CAP = 32                      # csrc/reseed_kernels.hip: the knob RESEED_CAP, forward entries per task in the first launch
MAX_TASK_STEPS, MAX_CASE_STEPS = 100_000, 2_000_000
TASK_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reseed_cases.npz")


def _long_world(at):
    return np.random.default_rng(20264).integers(0, 4, size=60_000).astype(np.uint8)


seed_cases.MORE_WORLDS["long"] = _long_world


def split_len_of(k, sf):
    """mem_collect_intv: (int)(min_seed_len * split_factor + .499), the product in float as C evaluates int * float"""
    return int(float(np.float32(k) * np.float32(sf)) + .499)


def factor_edge(k, want):
    """the two neighbouring floats (f0, f1) with split_len_of(k, f0) == want - 1 and split_len_of(k, f1) == want"""
    lo, hi = np.float32(1.0), np.float32(4.0)
    assert split_len_of(k, lo) < want <= split_len_of(k, hi)
    while np.nextafter(lo, np.float32(8)) < hi:
        mid = np.float32((float(lo) + float(hi)) / 2)
        if split_len_of(k, mid) < want:
            lo = mid
        else:
            hi = mid
    assert split_len_of(k, lo) == want - 1 and split_len_of(k, hi) == want
    return float(lo), float(hi)


# ---------------------------------------------------------------------------------------------------------------- one read, restated
class Walker:
    """the reference's interval arithmetic over the oracle's rank function"""

    def __init__(self, w):
        self.occ, self.fp = w.orc.lib.fmd_occ, C.byref(w.f)
        self.L2 = [int(w.f.L2[i]) for i in range(5)]
        self.primary = int(w.f.primary)

    def occ4(self, k):
        return [int(self.occ(self.fp, k & M64, c)) for c in range(4)]

    def start(self, b):                                      # bwt_set_intv
        L2 = self.L2
        return L2[b] + 1, L2[3 - b] + 1, L2[b + 1] - L2[b]

    def fwd(self, k, l, s, b):                               # bwt_extend(.., 0) and ok[3 - b]
        cb = 3 - b
        tk, tl = self.occ4(l - 1), self.occ4(l - 1 + s)
        ns = [tl[c] - tk[c] for c in range(4)]
        nk = [0] * 4
        nk[3] = k + (1 if l <= self.primary <= l + s - 1 else 0)
        nk[2] = nk[3] + ns[3]; nk[1] = nk[2] + ns[2]; nk[0] = nk[1] + ns[1]
        return nk[cb], self.L2[cb] + 1 + tk[cb], ns[cb]

    def bwd(self, k, s, c):                                  # bwt_extend(.., 1) and ok[c]: (k, s) alone, the list is walked backward only
        ol, ou = int(self.occ(self.fp, (k - 1) & M64, c)), int(self.occ(self.fp, k + s - 1, c))
        return self.L2[c] + ol + 1, ou - ol


def smem1a(W, q, x, m, msl):
    """bwt_smem1a(x, min_intv = m, max_intv = 0) -> (the x it returns, [(begin, end, k, s)] of at least msl bases, detail)"""
    n = len(q)
    assert q[x] < 4
    m = max(m, 1)
    k, l, s = W.start(int(q[x]))
    end, lst, at_push, steps, how = x + 1, [], [], 0, "end"
    i = x + 1
    while i < n:
        if q[i] < 4:
            nk, nl, ns = W.fwd(k, l, s, int(q[i])); steps += 1
            if ns != s:
                lst.append((k, s, end)); at_push.append(steps)
                if ns < m:
                    how = "small"
                    break
            k, l, s, end = nk, nl, ns, i + 1
        else:
            lst.append((k, s, end)); at_push.append(steps); how = "N"
            break
        i += 1
    if i == n:
        lst.append((k, s, end)); at_push.append(steps)
    ret, prev = lst[-1][2], lst[::-1]
    mem, rounds, equal, contained, behind, bwd_end = [], 0, 0, 0, 0, None
    for i in range(x - 1, -2, -1):
        c = -1 if i < 0 or q[i] > 3 else int(q[i])
        curr = []
        rounds += 1
        for pk, ps, pend in prev:
            if c >= 0:
                nk, ns = W.bwd(pk, ps, c); steps += 1
            if c < 0 or ns < m:
                if curr:
                    behind += 1                              # a longer match of this round is still growing
                elif not mem or i + 1 < mem[-1][0]:
                    mem.append((i + 1, pend, pk, ps))
                else:
                    contained += 1                           # the last one kept contains it
            elif not curr or ns != curr[-1][1]:
                curr.append((nk, ns, pend))
            else:
                equal += 1
        if not curr:
            bwd_end = "start" if i < 0 else ("N" if c < 0 else "empty")
            break
        prev = curr
    mem.reverse()
    out = [t for t in mem if t[1] - t[0] >= msl]
    d = SimpleNamespace(x=x, m=m, n_list=len(lst), fwd_end=how, rounds=rounds, bwd_end=bwd_end, steps=steps, equal=equal, contained=contained,
                        behind=behind, short=len(mem) - len(out), hits=out, at_push=at_push)
    return ret, out, d


def strategy1(W, q, msl, mi):
    """the third pass of mem_collect_intv: bwt_seed_strategy1 along the read -> ([(begin, end, k, s)], detail)"""
    n, x, seeds, steps = len(q), 0, [], 0
    d = SimpleNamespace(carry=0, at_min=[], end_unpushed=0, n_mid=0, empty_returned=0, calls=0)
    while x < n:
        if q[x] > 3:
            x += 1
            continue
        d.calls += 1
        k, l, s = W.start(int(q[x]))
        i, ret = x + 1, n
        while i < n:
            if q[i] > 3:
                ret = i + 1; d.n_mid += 1
                break
            if s == 0:
                nk = nl = ns = 0; d.carry += 1               # an empty interval stays empty: no rank query
            else:
                nk, nl, ns = W.fwd(k, l, s, int(q[i])); steps += 1
            if i - x == msl:
                d.at_min.append(ns)
            if ns < mi and i - x >= msl:
                if ns > 0:
                    seeds.append((x, i + 1, nk, ns))
                else:
                    d.empty_returned += 1
                ret = i + 1
                break
            k, l, s = nk, nl, ns
            i += 1
        else:
            d.end_unpushed += 1
        x = ret
    d.steps, d.seeds = steps, seeds
    return seeds, d


_read_cache = {}


def restate_read(w, q, msl, sf, sw, mi):
    """mem_collect_intv with re_seed for one read -> groups [(begin, end, k, s, round)] in the order of ks_introsort(mem_intv), the tasks' details, round 3's"""
    key = (w.name, q.tobytes(), msl, np.float32(sf).tobytes(), sw, mi)
    if key in _read_cache:
        return _read_cache[key]
    W = Walker(w)
    n, x, groups, steps1 = len(q), 0, [], 0
    while x < n:
        if q[x] < 4:
            x, got, d = smem1a(W, q, x, 1, msl)
            groups += [t + (1,) for t in got]; steps1 += d.steps
        else:
            x += 1
    split_len, tasks = split_len_of(msl, sf), []
    for b, e, _, s, _ in list(groups):
        if e - b < split_len or s > sw:
            continue
        _, got, d = smem1a(W, q, (b + e) >> 1, s + 1, msl)
        d.src = (b, e, s)
        tasks.append(d)
        groups += [t + (2,) for t in got]
    r3 = None
    if mi > 0:
        got, r3 = strategy1(W, q, msl, mi)
        groups += [t + (3,) for t in got]
    groups.sort(key=lambda t: (t[0], t[1]))
    out = SimpleNamespace(groups=groups, tasks=tasks, r3=r3, steps1=steps1)
    _read_cache[key] = out
    return out


def device_steps(S, cap=CAP):
    """the rank steps bmh_reseed_last_counts reports: round 2's lanes (a task whose list does not fit walks forward up to the push that does not fit, and
    the whole task again in the second launch) and round 3's"""
    return (sum(t.steps if t.n_list <= cap else t.steps + t.at_push[cap] for t in S.tasks), sum(d.r3.steps for d in S.reads if d.r3))


def columns(w, groups):
    """the columns of bmh_seeds_t for every read's groups in order (occurrences by suffix-array row), and the number of groups"""
    per_read = np.array([sum(g[3] for g in gs) for gs in groups], np.uint32)
    ns = int(per_read.sum())
    rbeg, qbeg, score = np.zeros(ns, np.uint64), np.zeros((ns, 2), np.int32), np.zeros(ns, np.uint32)
    o = 0
    for gs in groups:
        for b, e, k, s, _ in gs:
            rbeg[o:o + s] = [sa_of(w, k + u) for u in range(s)]
            qbeg[o:o + s] = (b, e); score[o] = s
            o += s
    prefix = np.zeros(len(per_read), np.uint32)
    prefix[1:] = np.cumsum(per_read)[:-1]
    return dict(rbeg=rbeg, qbeg=qbeg, score=score, n_ref_pos=per_read, prefix=prefix, n_smems=sum(len(gs) for gs in groups))


def restate(c):
    """a whole case: the tasks in (read, first-round order), per-read details, groups per round, and the columns of bmh_seeds_t"""
    w = world(c.genome)
    S = SimpleNamespace(reads=[], tasks=[], case=c)
    for r in range(len(c.lens)):
        d = restate_read(w, c.codes(r), c.msl, c.sf, c.sw, c.mi)
        S.reads.append(d)
        for t in d.tasks:
            S.tasks.append(SimpleNamespace(read=r, **vars(t)))
    S.n_tasks = len(S.tasks)
    S.lists = np.array([t.n_list for t in S.tasks], np.int64)
    S.n_over = int((S.lists > CAP).sum())
    S.rounds = tuple(sum(1 for d in S.reads for g in d.groups if g[4] == rd) for rd in (1, 2, 3))
    S.groups_per_read = np.array([len(d.groups) for d in S.reads], np.int64)
    S.r3_per_read = np.array([len(d.r3.seeds) if d.r3 else 0 for d in S.reads], np.int64)
    S.task_steps = np.array([t.steps for t in S.tasks], np.int64)
    S.steps = int(S.task_steps.sum()) + sum(d.r3.steps for d in S.reads if d.r3)
    S.cols = columns(w, [d.groups for d in S.reads])
    S.cols["rounds"] = np.array(S.rounds, np.int64)
    S.cols1 = columns(w, [[g for g in d.groups if g[4] == 1] for d in S.reads])          # re-seeding off: the first round alone
    return S


# ---------------------------------------------------------------------------------------------------------------- building cases
class RBatch(Batch):
    """the reads of one case with its options: min_seed_len, split_factor, split_width, max_mem_intv"""

    def __init__(self, name, family, msl=19, genome="main", sf=1.5, sw=10, mi=20):
        super().__init__(name, family, msl=msl, genome=genome)
        self.sf, self.sw, self.mi = float(np.float32(sf)), int(sw), int(mi)

    def tasks_of(self, q):
        return restate_read(self.w, np.asarray(q, np.uint8), self.msl, self.sf, self.sw, self.mi).tasks

    def case(self, must):
        assert len(self.reads) <= 300, self.name
        lens = np.array([len(r) for r in self.reads], np.uint32)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint32) if len(lens) else np.zeros(0, np.uint32)
        buf = np.concatenate(self.reads) if len(lens) and lens.sum() else np.zeros(0, np.uint8)
        return make_case(self.name, self.family, buf, offs, lens, self.msl, self.genome, (self.sf, self.sw, self.mi), must)


def selected(c):
    """rs_flag_in on the split pipeline's results (seed_cases.restate: every candidate in (read, ordinal) order, kept or filtered)"""
    R = c.R
    return R.kept & (R.e - R.beg >= split_len_of(c.msl, c.sf)) & (R.s_out <= c.sw)


def make_case(name, family, buf, offs, lens, msl, genome, opts, must):
    c = seed_cases.make_case(name, family, buf, offs, lens, msl, genome, 0, {"the first round": lambda c, R: True})
    c.sf, c.sw, c.mi = opts
    c.split_len = split_len_of(c.msl, c.sf)
    c.digest = hashlib.sha1((c.digest + repr((np.float32(c.sf).tobytes(), c.sw, c.mi))).encode()).hexdigest()
    c.S = S = restate(c)
    first = sorted((r,) + g[:4] for r, d in enumerate(S.reads) for g in d.groups if g[4] == 1)
    c.must = {what: bool(f(c, S)) for what, f in must.items()}
    assert c.must, name
    c.must["round 1 is the split pipeline's; as many tasks as selected results"] = first == sorted(c.R.smems) and int(selected(c).sum()) == S.n_tasks
    c.must["no task walks more than 100 000 rank steps, the case no more than 2 million"] = \
        int(S.task_steps.max(initial=0)) <= MAX_TASK_STEPS and S.steps <= MAX_CASE_STEPS and max((d.r3.steps for d in S.reads if d.r3), default=0) <= MAX_TASK_STEPS
    return c


def reseed_opt(c):
    """the case's options as bmh_seed_batch_reseed takes them"""
    from bwamem_hip.lib import ReseedOpt
    return ReseedOpt.default(enable=1, split_factor=c.sf, split_width=c.sw, max_mem_intv=c.mi)


def exact(B, i, L, at=40):
    """a 150-base read of unique genome with substitutions around [at, at + L): an SMEM of exactly L bases"""
    return sub(B.plain(i), at - 1, at + L)


def stair(B, m, lead=None):
    """lead . C . U[:m]: behind a lead of other genome the staircase's context and m bases of U (seed_cases: a task that starts inside U pushes at every base)"""
    w = B.w
    lead = B.plain(30, 30) if lead is None else lead
    return np.concatenate([lead, w.at["ctx"], w.at["U"][:m]]).astype(np.uint8)


def stair_with_list(B, n_list):
    """the shortest staircase read one of whose tasks has a forward list of n_list entries"""
    for m in range(30, 330):
        q = stair(B, m)
        if any(t.n_list == n_list for t in B.tasks_of(q)):
            return q
    raise AssertionError(n_list)


def lists_of(S, r):
    return [t.n_list for t in S.tasks if t.read == r]


def mer_head(B, cnt, front=()):
    """a read that begins (behind `front`) with the 40-mer planted cnt times: round 3's first extension has cnt occurrences at min_seed_len + 1 bases"""
    return np.concatenate([np.asarray(front, np.uint8), B.w.at["mers"][cnt], [2], 1 + B.rand(25) % 3]).astype(np.uint8)


# ---- select
def case_select_len(k, side):
    want = split_len_of(k, 1.5) + 1
    f = factor_edge(k, want)[side]
    sl = want - 1 + side
    B = RBatch("select_len_k%d_%s" % (k, ("below", "above")[side]), "select", msl=k, sf=f)
    lengths = (want - 2, want - 1, want, want + 1)
    for j, L in enumerate(lengths):
        B.add(exact(B, 2 * j, L, at=40)); B.add(exact(B, 2 * j + 1, L, at=41 + j))
    src = lambda S: sorted({t.src[1] - t.src[0] for t in S.tasks if t.src[0] >= 40 and t.src[1] < 100})
    return B.case({
        "int(%d * %.9g + .499) = %d, one more than with the float below" % (k, f, sl): lambda c, S: c.split_len == sl and split_len_of(k, factor_edge(k, want)[0]) == want - 1,
        "SMEMs of %d .. %d bases, tasks from %d up" % (lengths[0], lengths[-1], sl): lambda c, S: src(S) == [L for L in lengths if L >= sl] and
        {L for d in S.reads for g in d.groups if g[4] == 1 for L in [g[1] - g[0]]} >= set(lengths),
        "begin + end odd and even": lambda c, S: {(t.src[0] + t.src[1]) & 1 for t in S.tasks} == {0, 1}})


def case_select_filtered():
    B = RBatch("select_filtered", "select")
    for i in range(40):
        B.add(sub(B.plain(i), 45 + i % 7, 100 + i % 5))
        if i % 9 == 4:
            B.add(B.plain(50 + i, 25))

    def between(c, S):
        sel, R = selected(c), c.R
        t = np.flatnonzero(sel)
        return any(R.read[a] == R.read[b] and b - a > 1 and not R.kept[a + 1:b].any() for a, b in zip(t[:-1], t[1:]))
    return B.case({"filtered first-round results lie between two selected ones of a read": between,
                   "three tasks per long read, none for a 25-base read": lambda c, S: S.n_tasks == 120 and (c.lens == 25).sum() == 4,
                   "walks ended by ns < min_intv; no entry survives the backward rounds": lambda c, S: all(t.fwd_end == "small" and t.bwd_end == "empty" for t in S.tasks),
                   "hits shorter than min_seed_len are counted, not written": lambda c, S: sum(t.short for t in S.tasks) > 100 and S.rounds[1] == 0})


def case_tasks(n):
    B = RBatch("tasks_%d" % n, "select")
    have, i = 0, 0
    while have < n or i < 3:
        kind = i % 4
        q = (B.plain(i, 40), B.plain(i, 25), sub(B.plain(i), 48, 99), np.concatenate([B.plain(i, 27), [4], B.plain(i + 1, 40)]))[kind]
        if kind == 1 and i % 8 == 5:
            q = np.full(30, 4, np.uint8)
        nt = len(B.tasks_of(q))
        if have + nt > n:
            q = B.plain(i, 40) if have < n else B.plain(i, 25)
            nt = len(B.tasks_of(q))
        B.add(q); have += nt; i += 1
    return B.case({"%d tasks" % n: lambda c, S: S.n_tasks == n and S.n_over == 0,
                   "reads without a task between reads with tasks": lambda c, S: n == 0 or len({t.read for t in S.tasks}) < len(c.lens)})


# ---- round 2, forward
def case_list_edge():
    B = RBatch("list_32_33", "forward")
    B.add(B.plain(1, 40))
    for nl in (31, 32, 33, 34):
        B.add(stair_with_list(B, nl))
    B.add(sub(B.plain(2), 70))
    return B.case({"forward lists of exactly 32 entries (fits) and 33 (overflows)": lambda c, S: {31, 32, 33, 34} <= set(S.lists.tolist()) and S.n_over == 2,
                   "an overflowing task and a fitting one in the same wave": lambda c, S: 0 < S.n_over < S.n_tasks <= 64,
                   "the walks end on the read's end": lambda c, S: all(t.fwd_end == "end" for t in S.tasks if t.n_list >= 31),
                   "entries dropped for an equal size": lambda c, S: all(t.equal >= 30 for t in S.tasks if t.n_list >= 31)})


def twice(c, S):
    for d in S.reads:
        one = {g[:2] for g in d.groups if g[4] == 1}
        for g in d.groups:
            if g[4] == 2 and g[:2] in one and sum(1 for h in d.groups if h[:2] == g[:2]) >= 2:
                return True
    return False


def case_overflow(n, longest_elsewhere):
    B = RBatch("overflow_%d" % n, "forward")
    B.add(B.plain(99, 40))
    for i in range(n):
        B.add(stair(B, 60 + i % 6))
        if i % 16 == 3:
            B.add(B.plain(i, 40))
    B.add(B.plain(98, 60))
    if longest_elsewhere:
        B.add(sub(B.at(PLAIN_AT + 2000, 400), 100, 250))
    ovr = lambda S: {t.read for t in S.tasks if t.n_list > CAP}
    return B.case({"%d overflowing tasks" % n: lambda c, S: S.n_over == n and S.n_tasks > n,
                   "the batch's longest reads %s an overflowing task" % ("do not hold" if longest_elsewhere else "hold"):
                   lambda c, S: all((int(r) in ovr(S)) != longest_elsewhere for r in np.flatnonzero(c.lens == c.lens.max())),
                   "one overflowing task per staircase read, lists of 39 entries and more": lambda c, S: min(v for v in S.lists if v > CAP) == 39 and
                   len({v for v in S.lists.tolist() if v > CAP}) >= min(n, 3) and all(sum(v > CAP for v in lists_of(S, r)) == 1 for r in ovr(S))})


def case_overflow_all():
    """the staircase behind six bases: no task for the lead, the read's only task overflows; and the whole U"""
    B = RBatch("overflow_all", "forward")
    for i in range(5):
        B.add(stair(B, 70 + 9 * i, lead=B.plain(30, 30)[24:]))
    B.add(stair(B, 330, lead=B.plain(30, 30)[24:])); B.add(stair(B, 300, lead=B.plain(30, 30)[24:]))
    return B.case({"every task of the batch overflows": lambda c, S: S.n_over == S.n_tasks >= 7,
                   "a list of more than 256 entries": lambda c, S: int(S.lists.max()) > 256})


def case_forward_n():
    """an N inside U: the walk from the middle of the SMEM in front of it pushes at every base and ends on the N"""
    B = RBatch("forward_N", "forward")
    for at_u in (44, 47, 55, 70):
        q = stair(B, 90); q[42 + at_u] = 4
        B.add(q)
    B.add(stair(B, 62))
    q = B.plain(3); q[100] = 4
    B.add(q)
    return B.case({"walks ended by an N, of 32 entries or fewer and of more": lambda c, S: {t.n_list > CAP for t in S.tasks if t.fwd_end == "N"} == {False, True},
                   "walks ended by ns < min_intv and by the read's end beside them": lambda c, S: {t.fwd_end for t in S.tasks} == {"N", "small", "end"}})


def case_polya(n):
    """A^n on the small genome (an A-run of 2 000): with split_width 2 000 its one SMEM is a task that starts in the middle and pushes at every base"""
    B = RBatch("polyA_%d" % n, "forward", genome="small", sw=2000, mi=20)
    B.add(np.zeros(n, np.uint8)); B.add(B.at(100, 60)); B.add(np.zeros(40, np.uint8))
    return B.case({"one SMEM of %d occurrences, a task of min_intv %d" % (2001 - n, 2002 - n): lambda c, S: [(t.src, t.m) for t in S.tasks if t.read == 0] == [((0, n, 2001 - n), 2002 - n)],
                   "a list of %d entries in a second-launch column of %d" % (n // 2, n + 1): lambda c, S: lists_of(S, 0) == [n - n // 2] and int(c.lens.max()) == n,
                   "tens of thousands of rank steps in one lane": lambda c, S: 20_000 < int(S.task_steps.max()) <= MAX_TASK_STEPS,
                   "min_intv far beyond 65": lambda c, S: max(t.m for t in S.tasks) > 1000})


# ---- round 2, backward
def case_backward():
    """C U[:m] without a lead, split_width 2 000: the SMEM occurs 331 - m times, and the shorter entries of its task occur more often all the way back to the
    read's start, or to an N in front of C"""
    B = RBatch("backward_ends", "backward", sw=2000)
    none = np.zeros(0, np.uint8)
    for m in (40, 60, 100):
        B.add(stair(B, m, lead=none)); B.add(stair(B, m, lead=np.array([4], np.uint8))); B.add(stair(B, m, lead=np.concatenate([B.plain(9, 20), [4]])))
    B.add(stair(B, 80)); B.add(sub(B.plain(5), 60)); B.add(stair(B, 300))
    ends = lambda S: {t.bwd_end for t in S.tasks}
    return B.case({"backward rounds ended at the read's start, at an N and because no entry survives": lambda c, S: ends(S) == {"start", "N", "empty"},
                   "a round ends at position 0 of the read and at an N at position 0": lambda c, S: any(t.bwd_end == "N" and c.codes(t.read)[0] == 4 for t in S.tasks),
                   "entries dropped for an equal size": lambda c, S: sum(t.equal for t in S.tasks) > 100,
                   "hits dropped because the last one kept contains them": lambda c, S: sum(t.contained for t in S.tasks) > 0,
                   "hits shorter than min_seed_len": lambda c, S: sum(t.short for t in S.tasks) > 0,
                   "round-2 groups": lambda c, S: S.rounds[1] >= 6,
                   "a round-2 group equals a first-round group of its read: both stay": twice})


# ---- round 3
def case_r3_rows(mi):
    B = RBatch("r3_max_intv_%d" % mi, "round3", mi=mi)
    for i in range(6):
        B.add(sub(B.plain(i), 70))
    for cnt in MER_COUNTS:
        B.add(mer_head(B, cnt))
    must = {"round 2 runs": lambda c, S: S.n_tasks >= 6}
    if mi == 0:
        must["max_mem_intv 0: no third round"] = lambda c, S: S.rounds[2] == 0 and all(d.r3 is None for d in S.reads)
    else:
        must["max_mem_intv 1: every extension runs until its interval is empty, nothing passes"] = \
            lambda c, S: S.rounds[2] == 0 and sum(d.r3.empty_returned for d in S.reads) > 10 and sum(d.r3.steps for d in S.reads) > 500
    return B.case(must)


def case_r3_tiled(k):
    B = RBatch("r3_tiled_k%d" % k, "round3", msl=k)
    for i, ln in enumerate((200, 10 * (k + 1), 10 * (k + 1) + k, 10 * (k + 1) - 1, k + 1, k, 2 * (k + 1))):
        B.add(B.plain(3 * i, ln))
    full = lambda c, S, r: len(S.reads[r].r3.seeds) == int(c.lens[r]) // (k + 1) and all(e - b == k + 1 for b, e, _, _ in S.reads[r].r3.seeds)
    return B.case({"a read tiled by seeds of exactly k + 1 bases: len / (k + 1) of them, all its column holds": lambda c, S: all(full(c, S, r) for r in range(len(c.lens))),
                   "10 seeds on the 200-base read at k = 19": lambda c, S: k != 19 or len(S.reads[0].r3.seeds) == 10,
                   "the last seed ends on the read's last base": lambda c, S: S.reads[1].r3.seeds[-1][1] == c.lens[1] and S.reads[1].r3.end_unpushed == 0,
                   "an extension reaches the read's end unpushed": lambda c, S: S.reads[2].r3.end_unpushed == 1 and S.reads[3].r3.end_unpushed == 1,
                   "a read of k + 1 bases has one seed, one of k bases none": lambda c, S: len(S.reads[4].r3.seeds) == 1 and len(S.reads[5].r3.seeds) == 0})


def case_r3_edges():
    B = RBatch("r3_edges", "round3")
    N = np.array([4], np.uint8)
    p = B.plain(11, 100)
    B.add(np.concatenate([N, p]))                                # 0: N first
    B.add(np.concatenate([p, N]))                                # 1: N last
    q = p.copy(); q[10] = 4; q[50] = 4; B.add(q)                 # 2: an N in the middle of an extension, before and behind min_seed_len bases
    B.add(np.full(50, 4, np.uint8))                              # 3: only N
    B.add(np.zeros(0, np.uint8))                                 # 4: empty
    B.add(B.plain(12, 19)); B.add(B.plain(13, 1))                # 5, 6: shorter than k + 1
    B.add(B.rand(100))                                           # 7: from nowhere: the interval empties before k bases and is carried
    B.add(np.concatenate([B.rand(30), N, B.rand(15), N, N, B.plain(14, 45)]))    # 8
    B.add(np.concatenate([N, N, N]))                             # 9
    r3 = lambda S, r: S.reads[r].r3
    return B.case({"N first, N last, N in the middle of an extension, only N": lambda c, S: len(r3(S, 0).seeds) == 5 and len(r3(S, 1).seeds) == 5 and r3(S, 1).calls == 5 and r3(S, 2).n_mid == 2
                   and r3(S, 3).calls == 0 and r3(S, 9).calls == 0,
                   "an empty read and reads shorter than k + 1": lambda c, S: c.lens[4] == 0 and r3(S, 5).seeds == [] and r3(S, 5).end_unpushed == 1 and r3(S, 6).calls == 1,
                   "an interval that empties before k bases is carried without rank queries and returned empty": lambda c, S: r3(S, 7).carry > 20 and r3(S, 7).empty_returned >= 4
                   and r3(S, 7).seeds == [],
                   "a carried empty interval runs into an N and into the read's end": lambda c, S: r3(S, 8).carry > 0 and r3(S, 8).n_mid >= 2 and r3(S, 7).end_unpushed + r3(S, 8).end_unpushed >= 1,
                   "reads without any group between reads with groups": lambda c, S: S.groups_per_read[[2, 3, 4, 7, 8]].tolist()[1:4] == [0, 0, 0] and S.groups_per_read[2] > 0 and S.groups_per_read[8] > 0})


# ---- merge
def case_reads(n):
    """n reads, one lane of round 3 each; every third is without a group"""
    B = RBatch("reads_%d" % n, "merge")
    for i in range(n):
        if n > 2 and i % 3 == 1:
            B.add((B.rand(40), np.full(20, 4, np.uint8), np.zeros(0, np.uint8), B.plain(i, 18))[(i // 3) % 4])
        elif i % 3 == 2:
            B.add(sub(B.plain(i), 60 + i % 30))
        else:
            B.add(B.plain(i, 44 + i % 50))
    return B.case({"%d reads" % n: lambda c, S: len(c.lens) == n,
                   "groups of rounds 1 and 3": lambda c, S: S.rounds[0] >= (n + 2) // 3 and S.rounds[2] >= (n + 2) // 3,
                   "reads without any group between reads with groups": lambda c, S: n <= 2 or (int((S.groups_per_read == 0).sum()) == n // 3 + (n % 3 == 2) and S.groups_per_read[0] > 0
                                                                                                and S.groups_per_read[n - 1 - (n % 3 == 2)] > 0)})


def case_none():
    B = RBatch("no_group", "merge")
    for i in range(66):
        B.add((B.rand(30 + i), np.full(10 + i, 4, np.uint8), np.zeros(0, np.uint8), B.plain(i, i % 19))[i % 4])
    return B.case({"no group at all, no task": lambda c, S: sum(S.rounds) == 0 and S.n_tasks == 0,
                   "round 3 walks all the same": lambda c, S: sum(d.r3.steps for d in S.reads) > 100})


def case_long():
    """one read of 40 000 bases of the long genome with a substitution every few hundred bases, beside short ones"""
    B = RBatch("long_40000", "merge", genome="long")
    B.add(B.at(100, 60))
    r = B.at(10_000, 40_000)
    B.add(sub(r, *range(150, 40_000, 733)))
    B.add(B.at(55_000, 150))
    hi = lambda S: [g for g in S.reads[1].groups if g[0] > 32767]
    return B.case({"begin and end beyond 32 767 in the 16-bit key fields, from every round": lambda c, S: {g[4] for g in hi(S)} == {1, 2, 3} or
                   ({g[4] for g in hi(S)} == {1, 3} and S.rounds[1] == 0),
                   "ends beyond 39 000": lambda c, S: max(g[1] for g in S.reads[1].groups) > 39_000,
                   "2 000 round-3 seeds in one read": lambda c, S: len(S.reads[1].r3.seeds) >= 1900,
                   "tasks all along the read": lambda c, S: max(t.x for t in S.tasks) > 39_000 and len(lists_of(S, 1)) >= 50})


# ---- options
ROWS = {"a": ("below", 4, 4), "b": ("above", 5, 5), "c": (1.5, 63, 63), "d": (1.5, 64, 64), "e": (1.5, 65, 65), "f": (1.25, 129, 129), "g": (1.0, 130, 130)}


def case_options(k, row):
    f, sw, mi = ROWS[row]
    want = split_len_of(k, 1.5) + 1
    if isinstance(f, str):
        f = factor_edge(k, want)[f == "above"]
    sl = split_len_of(k, f)
    B = RBatch("options_k%d_%s" % (k, row), "options", msl=k, sf=f, sw=sw, mi=mi)
    for cnt in MER_COUNTS:
        B.add(mer_read(B, cnt)); B.add(mer_head(B, cnt)); B.add(mer_head(B, cnt, front=np.concatenate([B.plain(cnt, 10), [4]])))
    for j, L in enumerate((sl - 1, sl, sl + 1)):
        B.add(exact(B, 40 + j, L))
    B.add(stair(B, 75)); B.add(sub(B.plain(50), 75)); B.add(B.rand(50))
    mers = lambda S: {t.src[2] for t in S.tasks if t.src[1] - t.src[0] == 40 and t.src[2] > 1}
    at_min = lambda S: [v for d in S.reads for v in d.r3.at_min]
    pushed = lambda S: {s for d in S.reads for b, e, _, s in d.r3.seeds if e - b == k + 1}
    must = {"split_len %d: SMEMs of %d, %d and %d bases, the first is no task" % (sl, sl - 1, sl, sl + 1):
            lambda c, S: c.split_len == sl and {t.src[1] - t.src[0] for t in S.tasks if t.src[2] == 1 and 40 <= t.src[0] and t.src[1] < 100} == {sl, sl + 1},
            "split_width %d: the 40-mers of at most that many copies are tasks, no other" % sw: lambda c, S: mers(S) == {n for n in MER_COUNTS if n <= sw},
            "min_intv up to %d" % (max(n for n in MER_COUNTS if n <= sw) + 1): lambda c, S: max(t.m for t in S.tasks) == max(n for n in MER_COUNTS if n <= sw) + 1,
            "an overflowing task beside them": lambda c, S: S.n_over >= 1}
    if mi in MER_COUNTS:
        must["max_mem_intv %d: an interval of %d occurrences at k + 1 bases is extended further" % (mi, mi)] = lambda c, S: at_min(S).count(mi) >= 2 and mi not in pushed(S)
    if mi - 1 in MER_COUNTS:
        must["max_mem_intv %d: an interval of %d occurrences at k + 1 bases is a seed" % (mi, mi - 1)] = lambda c, S: at_min(S).count(mi - 1) >= 2 and mi - 1 in pushed(S)
    return B.case(must)


BUILDERS = {}
for _k in (15, 19, 23):
    for _s in (0, 1):
        BUILDERS["select_len_k%d_%s" % (_k, ("below", "above")[_s])] = functools.partial(case_select_len, _k, _s)
BUILDERS["select_filtered"] = case_select_filtered
for _n in TASK_COUNTS:
    BUILDERS["tasks_%d" % _n] = functools.partial(case_tasks, _n)
BUILDERS["list_32_33"] = case_list_edge
for _n, _e in ((1, False), (64, True), (65, False)):
    BUILDERS["overflow_%d" % _n] = functools.partial(case_overflow, _n, _e)
BUILDERS.update(overflow_all=case_overflow_all, forward_N=case_forward_n, polyA_600=functools.partial(case_polya, 600), backward_ends=case_backward)
for _m in (0, 1):
    BUILDERS["r3_max_intv_%d" % _m] = functools.partial(case_r3_rows, _m)
for _k in (15, 19, 23):
    BUILDERS["r3_tiled_k%d" % _k] = functools.partial(case_r3_tiled, _k)
BUILDERS["r3_edges"] = case_r3_edges
for _n in (1, 2, 63, 64, 65, 257):
    BUILDERS["reads_%d" % _n] = functools.partial(case_reads, _n)
BUILDERS.update(no_group=case_none, long_40000=case_long)
for _k in (15, 19, 23):
    for _r in ROWS:
        BUILDERS["options_k%d_%s" % (_k, _r)] = functools.partial(case_options, _k, _r)
NAMES = tuple(BUILDERS)
FAMILIES = ("select", "forward", "backward", "round3", "merge", "options")


@functools.lru_cache(maxsize=None)
def get(name):
    c = BUILDERS[name]()
    assert c.name == name
    return c


def all_cases():
    return {n: get(n) for n in NAMES}


# ---------------------------------------------------------------------------------------------------------------- the fixture
FIXTURE_KEYS = SEED_KEYS + ("n_smems", "rounds")


def reference_seeds(ref, bwts, c):
    """the compiled reference on a case (test_reseed.ref_seeds: mem_collect_intv over its own bwt_smem1, bwt_seed_strategy1 and bwt_sa): the columns
    common.assert_seeds_equal compares, the number of groups, and the groups per round"""
    from test_reseed import ref_seeds
    if c.genome not in bwts:
        bwts[c.genome] = ref.bwt_from_index(world(c.genome).idx)
    got = ref_seeds(ref, bwts[c.genome], c.all_codes, c.offs, c.lens, k=c.msl, reseed=dict(split_factor=c.sf, split_width=c.sw, max_mem_intv=c.mi))
    return {k: np.asarray(got[k]) for k in FIXTURE_KEYS}


def make_fixture(path=FIXTURE):
    """tests/golden/reseed_cases.npz from the reference's library (oracle/_ref/libref.so, where it can be built)"""
    import oracle_py
    oracle_py.build(ref=True)
    ref, bwts, z = oracle_py.Ref(), {}, {}
    for name, c in all_cases().items():
        for k, v in reference_seeds(ref, bwts, c).items():
            z[name + "." + k] = v.astype(np.uint32) if k == "rbeg" else v          # (every genome here is far below 2^31 bases)
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
            "tests/reseed_cases.py changed (%s): run reseed_cases.make_fixture() where the reference's library can be built" % name
        out[name] = {k: z[name + "." + k] for k in FIXTURE_KEYS}
        out[name]["rbeg"] = out[name]["rbeg"].astype(np.uint64)
        out[name]["n_smems"] = int(out[name]["n_smems"])
        for v in out[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    assert {f.split(".")[0] for f in z.files} == set(NAMES)
    return out


if __name__ == "__main__":
    print(make_fixture())
