"""The recalibration table's text: bam_recal's dict -> one tab-separated text whose lines begin with a section key, and back.

    AR name value                                        the run: min_qual, max_cycle, indel_quality, mismatch_context, indel_context, every read_group in table
                                                         order, every known_sites file, masked_positions
    SN name value                                        the summary words (RECAL_SUMMARY's names, without masked_positions)
    RG group event observations errors                   per group and event: the sums over qualities and cycles
    QS group quality event observations errors           per group, quality and event: the sums over cycles
    CY group quality cycle event observations errors
    CX group quality context event observations errors   the context `-` holds the bases whose context reaches before the read or over a base that is no ACGT

Rows with 0 observations are left out.  Groups come in table order, qualities and cycles ascending (negative cycles first), contexts in lexicographic order, events
M I D.  The tables by quality and by group are sums over the cycle table, made here and not on the device; read_recal_table checks them against the cycle rows."""
import numpy as np

from .lib import RECAL_INDEL_QUAL, RECAL_SUMMARY

EVENTS = ("M", "I", "D")
_BASES = "ACGT"


def recal_cycle(slot: int, max_cycle: int) -> int:
    """the cycle of a slot of the cycle tables: negative cycles first"""
    return slot - max_cycle if slot < max_cycle else slot - max_cycle + 1


def recal_cycle_slot(cycle: int, max_cycle: int) -> int:
    return max_cycle + cycle if cycle < 0 else max_cycle + cycle - 1


def _context_name(code: int, size: int) -> str:
    if code == 4 ** size:
        return "-"
    return "".join(_BASES[code >> (2 * (size - 1 - k)) & 3] for k in range(size))


def _context_code(name: str) -> int:
    if name == "-":
        return -1
    v = 0
    for ch in name:
        v = 4 * v + _BASES.index(ch)
    return v


def recal_event_tables(r: dict) -> dict:
    """bam_recal's dict -> the tables of every event as (observations, errors) pairs: "cycle" [groups][94][2 max_cycle][3 events][2] and "quality"
    [groups][94][3][2], "group" [groups][3][2] -- the sums over cycles --, "no_context" [groups][3][2]"""
    cm, ci = np.asarray(r["cycle_m"], dtype=np.uint64), np.asarray(r["cycle_id"], dtype=np.uint64)
    g, nq, nc = cm.shape[0], cm.shape[1], cm.shape[2]
    cyc = np.zeros((g, nq, nc, 3, 2), dtype=np.uint64)
    cyc[:, :, :, 0, :] = cm
    cyc[:, RECAL_INDEL_QUAL, :, 1, 0] = ci[:, :, 0]; cyc[:, RECAL_INDEL_QUAL, :, 1, 1] = ci[:, :, 1]
    cyc[:, RECAL_INDEL_QUAL, :, 2, 0] = ci[:, :, 0]; cyc[:, RECAL_INDEL_QUAL, :, 2, 1] = ci[:, :, 2]
    qual = cyc.sum(axis=2, dtype=np.uint64)
    xm, xi = np.asarray(r["context_m"], dtype=np.uint64), np.asarray(r["context_id"], dtype=np.uint64)
    none = np.zeros((g, 3, 2), dtype=np.uint64)
    none[:, 0, :] = xm[:, :, 16, :].sum(axis=1, dtype=np.uint64)
    none[:, 1, 0] = xi[:, 64, 0]; none[:, 1, 1] = xi[:, 64, 1]; none[:, 2, 0] = xi[:, 64, 0]; none[:, 2, 1] = xi[:, 64, 2]
    return dict(cycle=cyc, quality=qual, group=qual.sum(axis=1, dtype=np.uint64), no_context=none)


def recal_table_text(r: dict) -> str:
    """bam_recal's dict -> the text"""
    c = int(r["max_cycle"])
    groups = list(r["read_groups"])
    rows = [f"AR\tmin_qual\t{int(r['min_qual'])}", f"AR\tmax_cycle\t{c}", f"AR\tindel_quality\t{RECAL_INDEL_QUAL}", "AR\tmismatch_context\t2", "AR\tindel_context\t3"]
    rows += [f"AR\tread_group\t{g}" for g in groups]
    rows += [f"AR\tknown_sites\t{p}" for p in r.get("known_sites", [])]
    summary = [int(v) for v in r["summary"]]
    rows.append(f"AR\tmasked_positions\t{summary[RECAL_SUMMARY.index('masked_positions')]}")
    rows += [f"SN\t{nm}\t{summary[k]}" for k, nm in enumerate(RECAL_SUMMARY) if nm != "masked_positions"]
    t = recal_event_tables(r)
    cm, ci, xm, xi = (np.asarray(r[k]) for k in ("cycle_m", "cycle_id", "context_m", "context_id"))
    for gi, g in enumerate(groups):
        rows += [f"RG\t{g}\t{EVENTS[e]}\t{int(t['group'][gi, e, 0])}\t{int(t['group'][gi, e, 1])}" for e in range(3) if t["group"][gi, e, 0]]
    for gi, g in enumerate(groups):
        for q in np.flatnonzero(t["quality"][gi, :, :, 0].any(axis=1)):
            rows += [f"QS\t{g}\t{q}\t{EVENTS[e]}\t{int(t['quality'][gi, q, e, 0])}\t{int(t['quality'][gi, q, e, 1])}" for e in range(3) if t["quality"][gi, q, e, 0]]
    for gi, g in enumerate(groups):
        for q in np.flatnonzero(t["quality"][gi, :, :, 0].any(axis=1)):
            for s in np.flatnonzero(t["cycle"][gi, q, :, :, 0].any(axis=1)):
                rows += [f"CY\t{g}\t{q}\t{recal_cycle(int(s), c)}\t{EVENTS[e]}\t{int(t['cycle'][gi, q, s, e, 0])}\t{int(t['cycle'][gi, q, s, e, 1])}" for e in range(3) if t["cycle"][gi, q, s, e, 0]]
    for gi, g in enumerate(groups):
        for q in range(cm.shape[1]):
            got = [(_context_name(int(x), 2), 0, int(xm[gi, q, x, 0]), int(xm[gi, q, x, 1])) for x in np.flatnonzero(xm[gi, q, :, 0])]
            if q == RECAL_INDEL_QUAL:
                for x in np.flatnonzero(xi[gi, :, 0]):
                    got += [(_context_name(int(x), 3), e, int(xi[gi, x, 0]), int(xi[gi, x, e])) for e in (1, 2)]
            rows += [f"CX\t{g}\t{q}\t{nm}\t{EVENTS[e]}\t{o}\t{err}" for nm, e, o, err in sorted(got)]
    return "\n".join(rows) + "\n"


def write_recal_table(r: dict, dst) -> None:
    """recal_table_text to dst: a path or a text file object"""
    text = recal_table_text(r)
    if hasattr(dst, "write"):
        dst.write(text)
    else:
        with open(dst, "w") as f:
            f.write(text)


def recal_apply_report_text(a: dict) -> str:
    """the counts of the apply step (bam_apply_recal's dict) -> the report: rows `AS name value`, then `AQ quality before after` for every quality
    that bases held before or hold now"""
    from .lib import RECAL_APPLY_SUMMARY
    rows = [f"AS\t{nm}\t{int(a['summary'][k])}" for k, nm in enumerate(RECAL_APPLY_SUMMARY)]
    h = a["qual_hist"]
    rows += [f"AQ\t{q}\t{int(h[0][q])}\t{int(h[1][q])}" for q in range(len(h[0])) if int(h[0][q]) or int(h[1][q])]
    return "\n".join(rows) + "\n"


def write_recal_apply_report(a: dict, dst) -> None:
    """recal_apply_report_text to dst: a path or a text file object"""
    text = recal_apply_report_text(a)
    if hasattr(dst, "write"):
        dst.write(text)
    else:
        with open(dst, "w") as f:
            f.write(text)


def read_recal_table(path) -> dict:
    """the inverse of recal_table_text: a path (or the text's lines) -> bam_recal's dict.  ValueError names the line that is no row of the text, a row outside
    the run's parameters, or a QS / RG row that is not the sum of the cycle rows"""
    if isinstance(path, (list, tuple)):
        lines = list(path)
    else:
        with open(path) as f:
            lines = f.read().split("\n")
    ar = {"read_group": [], "known_sites": []}
    body = []
    for n, ln in enumerate(lines, 1):
        if not ln:
            continue
        f = ln.split("\t")
        if f[0] == "AR" and len(f) == 3:
            if f[1] in ("read_group", "known_sites"):
                ar[f[1]].append(f[2])
            else:
                ar[f[1]] = int(f[2])
        elif f[0] in ("SN", "RG", "QS", "CY", "CX"):
            body.append((n, f))
        else:
            raise ValueError(f"read_recal_table: line {n} is no row of a recalibration table: {ln!r}")
    for nm in ("min_qual", "max_cycle", "masked_positions"):
        if nm not in ar:
            raise ValueError(f"read_recal_table: no AR row {nm}")
    groups, c = ar["read_group"] or ["*"], int(ar["max_cycle"])
    gi = {g: k for k, g in enumerate(groups)}
    summary = np.zeros(16, dtype=np.uint64)
    summary[RECAL_SUMMARY.index("masked_positions")] = ar["masked_positions"]
    cm, ci = np.zeros((len(groups), 94, 2 * c, 2), dtype=np.uint64), np.zeros((len(groups), 2 * c, 3), dtype=np.uint64)
    xm, xi = np.zeros((len(groups), 94, 17, 2), dtype=np.uint64), np.zeros((len(groups), 65, 3), dtype=np.uint64)
    sums = []
    for n, f in body:
        try:
            if f[0] == "SN":
                summary[RECAL_SUMMARY.index(f[1])] = int(f[2])
                continue
            g, e, obs, err = gi[f[1]], EVENTS.index(f[-3]), int(f[-2]), int(f[-1])
            if f[0] in ("RG", "QS"):
                sums.append((n, g, int(f[2]) if f[0] == "QS" else None, e, obs, err))
                continue
            q = int(f[2])
            if e and q != RECAL_INDEL_QUAL:
                raise ValueError("an indel row at another quality than 45")
            if f[0] == "CY":
                cy = int(f[3])
                if cy == 0 or abs(cy) > c:
                    raise ValueError("a cycle outside the run's")
                s = recal_cycle_slot(cy, c)
                if e == 0:
                    cm[g, q, s] = (obs, err)
                else:
                    ci[g, s, 0] = obs; ci[g, s, e] = err
            else:
                x = _context_code(f[3])
                if len(f[3]) != (1 if x < 0 else 3 if e else 2):
                    raise ValueError("a context of another size than the event's")
                if e == 0:
                    xm[g, q, 16 if x < 0 else x] = (obs, err)
                else:
                    xi[g, 64 if x < 0 else x, 0] = obs; xi[g, 64 if x < 0 else x, e] = err
        except (KeyError, ValueError, IndexError) as ex:
            raise ValueError(f"read_recal_table: line {n}: {ex}") from None
    r = dict(summary=summary, cycle_m=cm, cycle_id=ci, context_m=xm, context_id=xi, min_qual=int(ar["min_qual"]), max_cycle=c, read_groups=groups, known_sites=ar["known_sites"])
    t = recal_event_tables(r)
    for n, g, q, e, obs, err in sums:
        want = t["group"][g, e] if q is None else t["quality"][g, q, e]
        if (int(want[0]), int(want[1])) != (obs, err):
            raise ValueError(f"read_recal_table: line {n}: the row is not the sum of the cycle rows ({int(want[0])} observations, {int(want[1])} errors)")
    return r


def recal_empirical_quality(observations, errors):
    """round(-10 log10((errors + 1) / (observations + 2))): the smoothed point estimate of a bin's quality -- a convenience for reading a table, not GATK 4's
    Bayesian empirical quality (which weighs the reported quality as a prior and is part of the report writer this project does not have)"""
    o, e = np.asarray(observations, dtype=np.float64), np.asarray(errors, dtype=np.float64)
    v = np.rint(-10.0 * np.log10((e + 1.0) / (o + 2.0))).astype(np.int64)
    return int(v) if v.ndim == 0 else v
