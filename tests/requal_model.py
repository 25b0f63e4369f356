"""Applying a recalibration table to the base qualities as a Python model, and the builders its tests share.  The deltas are made from the
definition in numpy doubles; a record is expanded into one entry per stored base -- the read in sequencing order with its cycles and contexts, mapped back to
the stored order --, not walked by index arithmetic as the library does, so the two share nothing but the definition."""
import struct

import numpy as np

from recal_model import ACGT, E_CUT, E_RG_ID, E_RG_NONE, E_RG_TYPE, E_TAGS, NQ, walk_tags

SEEN, REWRITTEN, NOQUAL, BASES, LOW, CHANGED, UNCHANGED, CAPPED, NOCTX = range(9)
WORDS = {E_TAGS: "has tags that cannot be walked to the record's end: the qualities are recalibrated by the read group its RG tag names",
         E_RG_NONE: "has no RG tag: the table to apply is kept per read group",
         E_RG_TYPE: "has an RG tag of another type than Z",
         E_RG_ID: "names a read group the table to apply does not hold",
         E_CUT: "is not whole: its bytes do not hold the fields, the name, the operations, the bases and the qualities it announces"}


def empty_table(groups=None, min_qual=6, max_cycle=500) -> dict:
    """a table without observations, in read_recal_table's form"""
    g = len(groups) if groups else 1
    return dict(cycle_m=np.zeros((g, NQ, 2 * max_cycle, 2), np.uint64), context_m=np.zeros((g, NQ, 17, 2), np.uint64), min_qual=min_qual, max_cycle=max_cycle,
                read_groups=list(groups) if groups else ["*"])


def slot(cycle: int, max_cycle: int) -> int:
    return max_cycle + cycle - 1 if cycle > 0 else max_cycle + cycle


def put(table, q, cycle, ctx, o, e, g=0) -> None:
    """o observations with e errors of quality q at `cycle` and context ctx (16: none) into both tables, so that their sums agree"""
    table["cycle_m"][g, q, slot(cycle, table["max_cycle"])] += np.array([o, e], np.uint64)
    table["context_m"][g, q, ctx] += np.array([o, e], np.uint64)


def emp(o, e):
    o, e = np.asarray(o, dtype=np.float64), np.asarray(e, dtype=np.float64)
    return np.minimum(93.0, -10.0 * np.log10((e + 1.0) / (o + 2.0)))


def deltas(table) -> np.ndarray:
    """the definition -> the fixed-point tables [groups][94][1 + 2 max_cycle + 16] (b, the cycle deltas, the context deltas) as int64"""
    cy, cx = np.asarray(table["cycle_m"], dtype=np.uint64), np.asarray(table["context_m"], dtype=np.uint64)
    g, c = cy.shape[0], int(table["max_cycle"])
    out = np.zeros((g, NQ, 1 + 2 * c + 16), np.int64)
    for k in range(g):
        oq, eq = cy[k, :, :, 0].sum(axis=1), cy[k, :, :, 1].sum(axis=1)
        og, eg = int(oq.sum()), int(eq.sum())
        dg = 0.0
        if og:
            expected = float((oq.astype(np.float64) * 10.0 ** (-np.arange(NQ) / 10.0)).sum())
            dg = float(emp(og, eg)) - -10.0 * np.log10(expected / og)
        B = np.where(oq > 0, emp(oq, eq), np.arange(NQ) + dg)
        B = np.clip(B, 1.0, 93.0)
        out[k, :, 0] = np.rint(256.0 * B)
        out[k, :, 1:1 + 2 * c] = np.where(cy[k, :, :, 0] > 0, np.rint(256.0 * (emp(cy[k, :, :, 0], cy[k, :, :, 1]) - B[:, None])), 0)
        out[k, :, 1 + 2 * c:] = np.where(cx[k, :, :16, 0] > 0, np.rint(256.0 * (emp(cx[k, :, :16, 0], cx[k, :, :16, 1]) - B[:, None])), 0)
    return out


def split(stream: bytes) -> list:
    out, p = [], 0
    while p < len(stream):
        n = struct.unpack_from("<I", stream, p)[0] + 4
        out.append(stream[p:p + n]); p += n
    return out


def apply_model(records, table, tabs=None):
    """records (a list or a stream) under `table`, whose fixed-point tables are `tabs` (None: deltas(table)) -> (the records rewritten, the counts: "summary" [16],
    "qual_hist" [2][94]), or ("refused", index, code) for the record with the smallest index that is refused"""
    if isinstance(records, (bytes, bytearray)):
        records = split(bytes(records))
    tabs = deltas(table) if tabs is None else np.asarray(tabs, dtype=np.int64)
    groups = [str(x) for x in (table.get("read_groups") or ["*"])]
    has_groups = groups != ["*"]
    min_qual, c = int(table["min_qual"]), int(table["max_cycle"])
    s, hist, out = np.zeros(16, np.int64), np.zeros((2, NQ), np.int64), []
    for index, rec in enumerate(records):
        s[SEEN] += 1
        if len(rec) < 36:
            return ("refused", index, E_CUT)
        l_name, n_ops, flag, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<H", rec, 18)[0], struct.unpack_from("<I", rec, 20)[0]
        seq_at = 36 + l_name + 4 * n_ops
        qual_at = seq_at + (l_seq + 1) // 2
        if qual_at + l_seq > len(rec):
            return ("refused", index, E_CUT)
        quals = list(rec[qual_at:qual_at + l_seq])
        if all(q == 0xff for q in quals):
            s[NOQUAL] += 1; out.append(rec)
            continue
        g = 0
        if has_groups:
            walked, _cg, ty, rg = walk_tags(rec[qual_at + l_seq:])
            if not walked:
                return ("refused", index, E_TAGS)
            if ty is None:
                return ("refused", index, E_RG_NONE)
            if ty != "Z":
                return ("refused", index, E_RG_TYPE)
            if rg.decode("latin-1") not in groups:
                return ("refused", index, E_RG_ID)
            g = groups.index(rg.decode("latin-1"))
        s[REWRITTEN] += 1; s[BASES] += l_seq
        # one entry per stored base, then the read as the machine saw it
        stored = [ACGT.get((rec[seq_at + i // 2] >> (0 if i & 1 else 4)) & 15, -1) for i in range(l_seq)]
        rev, neg = bool(flag & 0x10), flag & 0x81 == 0x81
        order = list(range(l_seq))[::-1] if rev else list(range(l_seq))                 # order[k]: the stored base that was read k-th
        read = [(-1 if stored[i] < 0 else 3 - stored[i]) if rev else stored[i] for i in order]
        new = list(quals)
        for k, i in enumerate(order):
            q0 = quals[i]
            hist[0, min(q0, 93)] += 1
            if q0 < min_qual:
                s[LOW] += 1; hist[1, min(q0, 93)] += 1
                continue
            cyc = k + 1
            if cyc > c:
                s[CAPPED] += 1; cyc = c
            cyc = -cyc if neg else cyc
            row = tabs[g, min(q0, 93)]
            v = int(row[0]) + int(row[1 + slot(cyc, c)])
            if k > 0 and read[k - 1] >= 0 and read[k] >= 0:
                v += int(row[1 + 2 * c + 4 * read[k - 1] + read[k]])
            else:
                s[NOCTX] += 1
            q1 = min(93, max(1, (v + 128) >> 8))                                        # (Python's >> floors, as an arithmetic shift does)
            new[i] = q1; hist[1, q1] += 1
            s[CHANGED if q1 != q0 else UNCHANGED] += 1
        out.append(rec[:qual_at] + bytes(new) + rec[qual_at + l_seq:])
    return out, dict(summary=s, qual_hist=hist)


def same_counts(got: dict, want: dict) -> bool:
    return np.array_equal(np.asarray(got["summary"], dtype=np.int64), want["summary"]) and np.array_equal(np.asarray(got["qual_hist"], dtype=np.int64), want["qual_hist"])


def random_table(seed=3, groups=None, min_qual=6, max_cycle=500, quals=(6, 7, 11, 25, 37, 40, 41), cycles=160) -> dict:
    """a table with observations at `quals` for cycles of both signs up to `cycles`, whose context rows sum to its cycle rows"""
    rng = np.random.default_rng(seed)
    t = empty_table(groups, min_qual, max_cycle)
    for g in range(t["cycle_m"].shape[0]):
        for q in quals:
            for sign in (1, -1):
                for cy in range(1, min(cycles, max_cycle) + 1):
                    if rng.random() < 0.1:
                        continue
                    o = int(rng.integers(1, 5000)); e = int(rng.integers(0, max(1, o // int(rng.integers(2, 2000))) + 1))
                    t["cycle_m"][g, q, slot(sign * cy, max_cycle)] = (o, e)
            o, e = (int(v) for v in t["cycle_m"][g, q].sum(axis=0))
            # the same observations and errors over the contexts: random shares, errors never above observations
            share = rng.multinomial(o, rng.dirichlet(np.ones(17)))
            errs = np.zeros(17, np.int64); left = e
            for x in rng.permutation(17):
                take = min(left, int(share[x])) if x == 16 else int(rng.integers(0, min(left, int(share[x])) + 1))
                errs[x] = take; left -= take
            for x in range(17):                                                           # (what the random shares left over)
                take = min(left, int(share[x] - errs[x])); errs[x] += take; left -= take
            assert left == 0
            t["context_m"][g, q, :, 0], t["context_m"][g, q, :, 1] = share, errs
    return t
