"""The recalibration table's definition as a Python model that follows it base by base, and the builders its tests share: records with real bases
and qualities, a small genome, its .pac body and its mask.  The model expands a record's operations into one entry per stored base -- not the cursor the library
walks --, so the two share nothing but the definition."""
import struct

import numpy as np

M, I, D, N, S, H, P, EQ, X = range(9)
NQ, INDEL_Q = 94, 45
SEEN, COUNTED, F_REF, F_FLAGS, F_MAPQ, F_NOQUAL, F_NOOPS, KEPT, SK_BASE, SK_QUAL, SK_MASK, SK_ANCHOR, CAPPED, MASKED = range(14)
E_SUM, E_PLACEHOLDER, E_SPAN, E_TAGS, E_RG_NONE, E_RG_TYPE, E_RG_ID, E_CUT = range(1, 9)
WORDS = {E_SUM: "has operations whose M I S = X lengths do not sum to its l_seq: the recalibration table walks them base by base",
         E_PLACEHOLDER: "holds the long-CIGAR placeholder (its operations are in its CG tag): the recalibration table reads the record's own operations",
         E_SPAN: "begins or ends outside its contig: the recalibration table compares it with the reference",
         E_TAGS: "has tags that cannot be walked to the record's end: the recalibration table reads RG and CG from them",
         E_RG_NONE: "has no RG tag: the recalibration table is kept per read group",
         E_RG_TYPE: "has an RG tag of another type than Z",
         E_RG_ID: "names a read group the table does not hold",
         E_CUT: "is not whole: its bytes do not hold the fields, the name, the operations, the bases and the qualities it announces"}
CODE4 = {"=": 0, "A": 1, "C": 2, "M": 3, "G": 4, "R": 5, "S": 6, "V": 7, "T": 8, "W": 9, "Y": 10, "H": 11, "K": 12, "D": 13, "B": 14, "N": 15}
ACGT = {1: 0, 2: 1, 4: 2, 8: 3}


def rrec(name=b"r", rid=0, pos=0, flag=0, mapq=30, ops=((10, M),), seq=None, qual=30, tag=b"", l_seq=None, nrid=-1, npos=-1, tlen=0) -> bytes:
    """a record built field by field (pos 0-based).  seq: a string over the BAM alphabet (None: A's); qual: one value for every base, a list, or None (0xff's)"""
    from test_bam_core import reg2bin
    if l_seq is None:
        l_seq = len(seq) if seq is not None else sum(n for n, o in ops if o in (M, I, S, EQ, X))
    if seq is None:
        seq = "A" * l_seq
    q = [0xff] * l_seq if qual is None else [qual] * l_seq if isinstance(qual, int) else list(qual)
    rl = sum(n for n, o in ops if o in (M, D, N, EQ, X))
    bin_ = 4680 if pos < 0 else reg2bin(pos, pos + 1 if (flag & 4) or rl == 0 else pos + rl)
    codes = [CODE4[c] for c in seq] + [0]
    packed = bytes(codes[2 * k] << 4 | codes[2 * k + 1] for k in range((l_seq + 1) // 2))
    body = struct.pack("<iiBBHHHIiii", rid, pos, len(name) + 1, mapq, bin_, len(ops), flag, l_seq, nrid, npos, tlen) + name + b"\0"
    body += b"".join(struct.pack("<I", n << 4 | o) for n, o in ops) + packed + bytes(q) + tag
    return struct.pack("<I", len(body)) + body


def pack_pac(codes) -> bytes:
    """2-bit codes -> the .pac body: 4 bases a byte, the first in the top bits"""
    c = np.concatenate([np.asarray(codes, dtype=np.uint8), np.zeros(4, np.uint8)])
    n = (len(codes) + 3) // 4
    c = c[:4 * n].reshape(n, 4)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8).tobytes() + b"\0"


def mask_words(bits) -> np.ndarray:
    """a boolean array over the genome -> the mask's uint64 words"""
    b = np.asarray(bits, dtype=bool)
    pad = np.zeros((len(b) + 63) // 64 * 64, dtype=bool); pad[:len(b)] = b
    return np.packbits(pad, bitorder="little").view("<u8").astype(np.uint64)


def walk_tags(t: bytes):
    """the tags by their types -> (walked, has CG:B,I, the first RG tag's type or None, its value)"""
    p, cg, rg_type, rg = 0, False, None, None
    sizes = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while p < len(t):
        if len(t) - p < 3:
            return False, cg, rg_type, rg
        key, ty = t[p:p + 2], chr(t[p + 2])
        p += 3
        if ty in sizes:
            ln = sizes[ty]
        elif ty in "ZH":
            e = t.find(b"\0", p)
            if e < 0:
                return False, cg, rg_type, rg
            ln = e + 1 - p
        elif ty == "B":
            if len(t) - p < 5:
                return False, cg, rg_type, rg
            sub = chr(t[p])
            if sub not in "cCsSiIf":
                return False, cg, rg_type, rg
            if key == b"CG" and sub == "I":
                cg = True
            ln = 5 + sizes[sub] * struct.unpack_from("<I", t, p + 1)[0]
        else:
            return False, cg, rg_type, rg
        if ln > len(t) - p:
            return False, cg, rg_type, rg
        if key == b"RG" and rg_type is None:
            rg_type, rg = ty, (t[p:p + ln - 1] if ty == "Z" else None)
        p += ln
    return True, cg, rg_type, rg


def empty_result(n_groups: int, max_cycle: int) -> dict:
    """(int64 while the model adds to it: numpy adds Python integers to those exactly)"""
    return dict(summary=np.zeros(16, np.int64), cycle_m=np.zeros((n_groups, NQ, 2 * max_cycle, 2), np.int64), cycle_id=np.zeros((n_groups, 2 * max_cycle, 3), np.int64),
                context_m=np.zeros((n_groups, NQ, 17, 2), np.int64), context_id=np.zeros((n_groups, 65, 3), np.int64))


def model(records, contig_len, ref, mask=None, groups=None, min_qual=6, max_cycle=500):
    """the definition, base by base.  records: a list of records (or a stream); ref: the genome's 2-bit codes, the contigs back to back; mask: a boolean array
    over it (or None).  -> bam_recal's arrays, or ("refused", index, code) for the record with the smallest index that is refused"""
    if isinstance(records, (bytes, bytearray)):
        from test_bam_sort import split_records
        records = split_records(bytes(records))
    starts = np.concatenate([[0], np.cumsum(contig_len)]).astype(np.int64)
    ids = [g.encode() if isinstance(g, str) else g for g in groups] if groups else None
    out = empty_result(len(ids) if ids else 1, max_cycle)
    sm = out["summary"]
    sm[MASKED] = int(np.count_nonzero(mask)) if mask is not None else 0
    for index, r in enumerate(records):
        if len(r) < 36:
            return ("refused", index, E_CUT)
        rid, pos, l_name, mapq, _bin, n_ops, fl, l_seq, _nrid, _npos, _tlen = struct.unpack_from("<iiBBHHHIiii", r, 4)
        sm[SEEN] += 1
        if not 0 <= rid < len(contig_len):
            sm[F_REF] += 1; continue
        if fl & (0x4 | 0x100 | 0x200 | 0x400):
            sm[F_FLAGS] += 1; continue
        if mapq in (0, 255):
            sm[F_MAPQ] += 1; continue
        p = 36 + l_name
        seq_at = p + 4 * n_ops
        qual_at = seq_at + (l_seq + 1) // 2
        if qual_at + l_seq > len(r):
            return ("refused", index, E_CUT)
        ops = [(v >> 4, v & 15) for v in struct.unpack_from(f"<{n_ops}I", r, p)]
        quals = r[qual_at:qual_at + l_seq]
        if all(q == 0xff for q in quals):
            sm[F_NOQUAL] += 1; continue
        if not ops:
            sm[F_NOOPS] += 1; continue
        if sum(n for n, o in ops if o in (M, I, S, EQ, X)) != l_seq:
            return ("refused", index, E_SUM)
        walked, cg, rg_type, rg = walk_tags(r[qual_at + l_seq:])
        if walked and cg and len(ops) == 2 and ops[0] == (l_seq, S) and ops[1][1] == N:
            return ("refused", index, E_PLACEHOLDER)
        if pos < 0 or pos + sum(n for n, o in ops if o in (M, D, N, EQ, X)) > contig_len[rid]:
            return ("refused", index, E_SPAN)
        if not walked:
            return ("refused", index, E_TAGS)
        g = 0
        if ids:
            if rg_type is None:
                return ("refused", index, E_RG_NONE)
            if rg_type != "Z":
                return ("refused", index, E_RG_TYPE)
            if rg not in ids:
                return ("refused", index, E_RG_ID)
            g = ids.index(rg)
        sm[COUNTED] += 1
        # one entry per stored base: its class, its reference position (M: its own; I: the one before the operation, None before the contig), a D in front of it
        cls, rpos, d_before = [], [], []
        at, pending = pos, False
        for n, o in ops:
            if o in (M, EQ, X):
                for k in range(n):
                    cls.append("M"); rpos.append(at + k); d_before.append(pending); pending = False
                at += n
            elif o == I:
                for k in range(n):
                    cls.append("I"); rpos.append(at - 1 if at > 0 else None); d_before.append(pending); pending = False
            elif o == S:
                for k in range(n):
                    cls.append("S"); rpos.append(None); d_before.append(pending); pending = False
            elif o == D:
                pending = pending or n > 0; at += n
            elif o == N:
                at += n
        d_after = d_before[1:] + [pending]
        clips = [(n, o) for n, o in ops if n and o not in (H, P)]
        lead = 0
        while clips and clips[0][1] == S:
            lead += clips.pop(0)[0]
        trail = 0
        while clips and clips[-1][1] == S:
            trail += clips.pop()[0]
        n_kept = l_seq - lead - trail
        sm[KEPT] += n_kept
        code4 = [(r[seq_at + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(l_seq)]
        rev, neg = bool(fl & 0x10), fl & 0x81 == 0x81
        kept = [ACGT.get(c, -1) for c in code4[lead:lead + n_kept]]
        order = [3 - c if c >= 0 else -1 for c in reversed(kept)] if rev else kept
        for i in range(lead, lead + n_kept):
            c = ACGT.get(code4[i], -1)
            if c < 0:
                sm[SK_BASE] += 1; continue
            if quals[i] < min_qual:
                sm[SK_QUAL] += 1; continue
            snp = False
            if cls[i] == "M":
                gp = int(starts[rid]) + rpos[i]
                if mask is not None and mask[gp]:
                    sm[SK_MASK] += 1; continue
                snp = int(ref[gp]) != c
            elif cls[i] == "I" and rpos[i] is not None and mask is not None and mask[int(starts[rid]) + rpos[i]]:
                sm[SK_ANCHOR] += 1; continue
            if not rev:
                ins = cls[i] != "I" and i + 1 < l_seq and cls[i + 1] == "I"
                dele = d_after[i]
            else:
                ins = cls[i] != "I" and i >= 1 and cls[i - 1] == "I"
                dele = d_before[i]
            k = lead + n_kept - 1 - i if rev else i - lead
            cyc = k + 1
            if cyc > max_cycle:
                sm[CAPPED] += 1; cyc = max_cycle
            slot = max_cycle - cyc if neg else max_cycle + cyc - 1
            q = min(quals[i], NQ - 1)
            b0, b1, b2 = order[k], order[k - 1] if k >= 1 else -1, order[k - 2] if k >= 2 else -1
            mctx = 16 if b1 < 0 else 4 * b1 + b0
            ictx = 64 if b1 < 0 or b2 < 0 else 16 * b2 + 4 * b1 + b0
            out["cycle_m"][g, q, slot] += (1, snp); out["context_m"][g, q, mctx] += (1, snp)
            out["cycle_id"][g, slot] += (1, ins, dele); out["context_id"][g, ictx] += (1, ins, dele)
    return out


ARRAYS = ("summary", "cycle_m", "cycle_id", "context_m", "context_id")


def equal(a: dict, b: dict) -> bool:
    return all(np.array_equal(np.asarray(a[k], dtype=np.uint64), np.asarray(b[k], dtype=np.uint64)) for k in ARRAYS)


def check_invariants(r: dict, kept_of_counted=None) -> None:
    """what holds for every result: I and D share their observations (by layout); errors <= observations; the sums over cycles are the sums over contexts
    and `none`; M observations + skipped bases = the kept bases of the counted records"""
    cm, ci, xm, xi, sm = (np.asarray(r[k]).astype(np.int64) for k in ("cycle_m", "cycle_id", "context_m", "context_id", "summary"))
    assert (cm[..., 1] <= cm[..., 0]).all() and (xm[..., 1] <= xm[..., 0]).all()
    assert (ci[..., 1] <= ci[..., 0]).all() and (ci[..., 2] <= ci[..., 0]).all() and (xi[..., 1] <= xi[..., 0]).all() and (xi[..., 2] <= xi[..., 0]).all()
    assert np.array_equal(cm.sum(axis=2), xm.sum(axis=2)) and np.array_equal(ci.sum(axis=1), xi.sum(axis=1))
    assert np.array_equal(cm[..., 0].sum(axis=(1, 2)), ci[..., 0].sum(axis=1))
    assert cm[..., 0].sum() + sm[SK_BASE:SK_ANCHOR + 1].sum() == sm[KEPT]
    assert sm[SEEN] == sm[COUNTED] + sm[F_REF:F_NOOPS + 1].sum()
    if kept_of_counted is not None:
        assert sm[KEPT] == kept_of_counted


def genome(seed=5, lens=(2600, 1700), hole=(900, 40)):
    """a small random genome of two contigs with one hole: (contigs, 2-bit codes, pac bytes, the hole as (offset, length) in pac)"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=sum(lens), dtype=np.uint8)
    return [("c1", lens[0]), ("c2", lens[1])], ref, pack_pac(ref), hole


def synth_records(n, contigs, ref, seed=9, groups=None, read_len=(30, 151), quals=(2, 3, 5, 6, 7, 11, 25, 37, 40, 41)):
    """n records cut from the genome with planted mismatches, insertions, deletions, clips and N bases, both strands, pairs' first and second reads, and some
    records of every kind that is left out"""
    rng = np.random.default_rng(seed)
    starts = np.concatenate([[0], np.cumsum([c[1] for c in contigs])])
    out = []
    for k in range(n):
        rid = int(rng.integers(0, len(contigs)))
        L = int(rng.integers(*read_len))
        ops, seq, at = [], [], 0
        pos = int(rng.integers(0, contigs[rid][1] - 2 * L - 8))
        if rng.random() < 0.3:
            c = int(rng.integers(1, 9)); ops.append((c, S)); seq += list(rng.integers(0, 4, c))
        left = L
        while left > 0:
            m = int(min(left, rng.integers(1, 60)))
            ops.append((m, M if rng.random() < 0.9 else (EQ if rng.random() < 0.5 else X)))
            seq += list(ref[starts[rid] + pos + at:starts[rid] + pos + at + m]); at += m; left -= m
            if left > 0:
                w = rng.random()
                if w < 0.3:
                    c = int(rng.integers(1, 4)); ops.append((c, I)); seq += list(rng.integers(0, 4, c))
                elif w < 0.6:
                    c = int(rng.integers(1, 5)); ops.append((c, D)); at += c
                elif w < 0.65:
                    c = int(rng.integers(1, 6)); ops.append((c, N)); at += c
        if rng.random() < 0.3:
            c = int(rng.integers(1, 9)); ops.append((c, S)); seq += list(rng.integers(0, 4, c))
        if rng.random() < 0.1:
            ops = [(3, H)] + ops
        seq = np.array(seq, dtype=np.int64)
        flip = rng.random(len(seq)) < 0.02
        seq[flip] = (seq[flip] + 1 + rng.integers(0, 3, int(flip.sum()))) % 4
        letters = ["ACGT"[c] for c in seq]
        for j in np.flatnonzero(rng.random(len(seq)) < 0.01):
            letters[j] = "N"
        flag = (0x10 if rng.random() < 0.5 else 0) | int(rng.choice([0, 0x41, 0x81, 0x81 | 0x20]))
        mapq, qual = int(rng.integers(1, 61)), [int(x) for x in rng.choice(quals, len(seq))]
        w = rng.random()
        if w < 0.03:
            flag |= int(rng.choice([0x4, 0x100, 0x200, 0x400]))
        elif w < 0.05:
            mapq = int(rng.choice([0, 255]))
        elif w < 0.06:
            qual = None
        elif w < 0.07:
            rid = -1
        elif w < 0.09:
            flag |= 0x800
        tag = b"NMC\x01" + (b"RGZ" + groups[int(rng.integers(0, len(groups)))].encode() + b"\0" if groups else b"") + b"XSi\x05\0\0\0"
        out.append(rrec(b"q%d" % k, rid, pos, flag, mapq, tuple(ops), "".join(letters), qual, tag))
    return out


# ---------------------------------------------------------------------------------------------------------------- the table of cases, counted by hand

# a reference small enough to count by hand: c1 = ACGT five times, c2 = GGGGCCCCAAAA
SMALL_LENS = [20, 12]
SMALL_CONTIGS = [("c1", 20), ("c2", 12)]
SMALL_REF = np.array([p % 4 for p in range(20)] + [2] * 4 + [1] * 4 + [0] * 4, dtype=np.uint8)
SMALL_PAC = pack_pac(SMALL_REF)


def _mask_at(*positions):
    m = np.zeros(32, bool)
    m[list(positions)] = True
    return m


def expect_rows(obs, group="*"):
    """the CY and CX rows of the text for observations listed by hand, one tuple per observed base: (quality, cycle, mismatch context, indel context, snp, ins, del)
    -- the contexts as the text writes them, `-` for none"""
    cy, cx = {}, {}
    for q, cyc, mc, ic, snp, ins, dele in obs:
        for table, key, err in ((cy, (q, cyc, 0), snp), (cy, (INDEL_Q, cyc, 1), ins), (cy, (INDEL_Q, cyc, 2), dele), (cx, (q, mc, 0), snp), (cx, (INDEL_Q, ic, 1), ins), (cx, (INDEL_Q, ic, 2), dele)):
            o, e = table.get(key, (0, 0))
            table[key] = (o + 1, e + err)
    return ["CY\t%s\t%d\t%d\t%s\t%d\t%d" % (group, q, c, "MID"[ev], o, e) for (q, c, ev), (o, e) in sorted(cy.items())] + \
           ["CX\t%s\t%d\t%s\t%s\t%d\t%d" % (group, q, c, "MID"[ev], o, e) for (q, c, ev), (o, e) in sorted(cx.items())]


def hand_cases():
    """(name, records, mask or None, keywords, the observations counted by hand) -- one record for every branch of the definition.  c1 reads ACGT ACGT ...: the
    base at position p is "ACGT"[p % 4]"""
    c = []
    # 2S 3M at c1:4, forward: the kept bases ACG match; the clipped T's are no context (it reaches before the first kept base) and no cycle
    c.append(("soft clip in front", [rrec(b"a", 0, 4, 0, 30, ((2, S), (3, M)), "TTACG", 30)], None, {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 2, "AC", "-", 0, 0, 0), (30, 3, "CG", "ACG", 0, 0, 0)]))
    # 3M 2S at c1:4, 0x10: sequencing order is the reverse complement of the kept ACG: C G T, cycles 1 2 3
    c.append(("soft clip behind, reverse", [rrec(b"b", 0, 4, 0x10, 30, ((3, M), (2, S)), "ACGTT", 30)], None, {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 2, "CG", "-", 0, 0, 0), (30, 3, "GT", "CGT", 0, 0, 0)]))
    # 1S 3M 2S, 0x10 and the second of a pair: the same bases, cycles -1 -2 -3 -- the clips at either end are not counted in
    c.append(("soft clips at both ends, reverse second read", [rrec(b"c", 0, 4, 0x91, 30, ((1, S), (3, M), (2, S)), "TACGTT", 30)], None, {},
              [(30, -1, "-", "-", 0, 0, 0), (30, -2, "CG", "-", 0, 0, 0), (30, -3, "GT", "CGT", 0, 0, 0)]))
    # 5H 3M 2H: hard clips take nothing
    c.append(("hard clips", [rrec(b"d", 0, 4, 0, 30, ((5, H), (3, M), (2, H)), "ACG", 30)], None, {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 2, "AC", "-", 0, 0, 0), (30, 3, "CG", "ACG", 0, 0, 0)]))
    # 2M 3N 2M at c1:0: AC, then positions 5 6 = CG; N advances the reference only and is no deletion
    c.append(("N", [rrec(b"e", 0, 0, 0, 30, ((2, M), (3, N), (2, M)), "ACCG", 30)], None, {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 2, "AC", "-", 0, 0, 0), (30, 3, "CC", "ACC", 0, 0, 0), (30, 4, "CG", "CCG", 0, 0, 0)]))
    # 2= 2X with ATGT against ACGT: the second base differs under `=`, the last two match under `X` -- the bases decide
    c.append(("= and X are not trusted", [rrec(b"f", 0, 0, 0, 30, ((2, EQ), (2, X)), "ATGT", 30)], None, {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 2, "AT", "-", 1, 0, 0), (30, 3, "TG", "ATG", 0, 0, 0), (30, 4, "GT", "TGT", 0, 0, 0)]))
    # ACNTAC: the N is skipped; the mismatch context of T and the indel contexts of T and A reach over it
    c.append(("a base that is no ACGT inside a context", [rrec(b"g", 0, 0, 0, 30, ((6, M),), "ACNTAC", 30)], None, {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 2, "AC", "-", 0, 0, 0), (30, 4, "-", "-", 0, 0, 0), (30, 5, "TA", "-", 0, 0, 0), (30, 6, "AC", "TAC", 0, 0, 0)]))
    # ACGT at c1:4 with position 5 masked: the C is skipped, and stays a base of its neighbours' contexts
    c.append(("a masked M position", [rrec(b"h", 0, 4, 0, 30, ((4, M),), "ACGT", 30)], _mask_at(5), {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 3, "CG", "ACG", 0, 0, 0), (30, 4, "GT", "CGT", 0, 0, 0)]))
    # 2M 2I 2M at c1:4 with position 5 masked: the C (position 5) and both inserted bases (their anchor is position 5) are skipped -- and with the C the ins event
    c.append(("a masked insertion anchor", [rrec(b"i", 0, 4, 0, 30, ((2, M), (2, I), (2, M)), "ACTTGT", 30)], _mask_at(5), {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 5, "TG", "TTG", 0, 0, 0), (30, 6, "GT", "TGT", 0, 0, 0)]))
    # a hole of the reference (c2's first four bases) is masked like a known site: GGCC at c2:2 keeps its CC
    c.append(("a hole", [rrec(b"j", 1, 2, 0, 30, ((4, M),), "GGCC", 30)], _mask_at(20, 21, 22, 23), {},
              [(30, 3, "GC", "GGC", 0, 0, 0), (30, 4, "CC", "GCC", 0, 0, 0)]))
    # the cap: cycles above it share it
    c.append(("cap 2", [rrec(b"k", 0, 0, 0, 30, ((3, M),), "ACG", 30)], None, dict(max_cycle=2),
              [(30, 1, "-", "-", 0, 0, 0), (30, 2, "AC", "-", 0, 0, 0), (30, 2, "CG", "ACG", 0, 0, 0)]))
    c.append(("cap 1, reverse second read", [rrec(b"l", 0, 4, 0x91, 30, ((3, M),), "ACG", 30)], None, dict(max_cycle=1),
              [(30, -1, "-", "-", 0, 0, 0), (30, -1, "CG", "-", 0, 0, 0), (30, -1, "GT", "CGT", 0, 0, 0)]))
    c.append(("a read of one base", [rrec(b"m", 1, 0, 0, 30, ((1, M),), "G", 30)], None, {}, [(30, 1, "-", "-", 0, 0, 0)]))
    # 1S 1I 3M at c1:4: the inserted T is the first kept base.  Forward: the base before the run is the clip, the event is dropped
    c.append(("I at the first kept base", [rrec(b"n", 0, 4, 0, 30, ((1, S), (1, I), (3, M)), "TTACG", 30)], None, {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 2, "TA", "-", 0, 0, 0), (30, 3, "AC", "TAC", 0, 0, 0), (30, 4, "CG", "ACG", 0, 0, 0)]))
    # ... 0x10: the base behind the run (the A) carries it; sequencing order is the reverse complement of TACG: C G T A
    c.append(("I at the first kept base, reverse", [rrec(b"o", 0, 4, 0x10, 30, ((1, S), (1, I), (3, M)), "TTACG", 30)], None, {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 2, "CG", "-", 0, 0, 0), (30, 3, "GT", "CGT", 0, 1, 0), (30, 4, "TA", "GTA", 0, 0, 0)]))
    # 3M 1D at c1:4: forward, the last kept base carries the deletion behind it; 0x10, no base lies behind it
    c.append(("D behind the last kept base", [rrec(b"p", 0, 4, 0, 30, ((3, M), (1, D)), "ACG", 30)], None, {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 2, "AC", "-", 0, 0, 0), (30, 3, "CG", "ACG", 0, 0, 1)]))
    c.append(("D behind the last kept base, reverse", [rrec(b"q", 0, 4, 0x10, 30, ((3, M), (1, D)), "ACG", 30)], None, {},
              [(30, 1, "-", "-", 0, 0, 0), (30, 2, "CG", "-", 0, 0, 0), (30, 3, "GT", "CGT", 0, 0, 0)]))
    # qualities 5 6 7 around min_qual 6: the first base is skipped
    c.append(("qualities around min_qual", [rrec(b"r", 0, 0, 0, 30, ((3, M),), "ACG", [5, 6, 7])], None, {},
              [(6, 2, "AC", "-", 0, 0, 0), (7, 3, "CG", "ACG", 0, 0, 0)]))
    return c


def table_cases():
    """(name, records, mask or None, keywords): the hand-counted cases and the other cases of the table -- events at both ends in both strands, runs of I around a D,
    an insertion in front of the contig, every reason a record is left out for"""
    out = [(nm, recs, mask, kw) for nm, recs, mask, kw, _obs in hand_cases()]
    for flag in (0, 0x10, 0x91):
        out.append(("events at the ends, flag %#x" % flag, [
            rrec(b"i1", 0, 4, flag, 30, ((1, S), (1, I), (3, M)), "TTACG", 30), rrec(b"i2", 0, 4, flag, 30, ((3, M), (1, I), (1, S)), "ACGTT", 30),
            rrec(b"d1", 0, 4, flag, 30, ((1, D), (3, M)), "CGT", 30), rrec(b"d2", 0, 4, flag, 30, ((3, M), (1, D)), "ACG", 30),
            rrec(b"ii", 0, 0, flag, 30, ((2, M), (1, I), (1, I), (1, D), (1, I), (2, M)), "ACTTTGT", 30), rrec(b"dn", 0, 0, flag, 30, ((2, M), (1, D), (2, N), (2, M)), "ACCG", 30),
            rrec(b"sd", 0, 4, flag, 30, ((2, S), (1, D), (2, M), (1, I), (1, D), (2, M), (3, S)), "TTCGTACGGG", 30),
            rrec(b"hs", 0, 4, flag, 30, ((5, H), (1, S), (3, M), (1, S), (2, H)), "TACGT", 30), rrec(b"all", 0, 4, flag, 30, ((4, S),), "ACGT", 30)], _mask_at(9), {}))
    out.append(("an insertion in front of the contig", [rrec(b"i0", 0, 0, 0, 30, ((2, I), (2, M)), "TTAC", 30)], np.ones(32, bool), {}))
    out.append(("a masked anchor behind a D", [rrec(b"ad", 0, 4, 0, 30, ((2, M), (1, D), (1, I), (2, M)), "ACTTA", 30)], _mask_at(6), {}))
    out.append(("qualities above 93", [rrec(b"q", 0, 0, 0, 30, ((3, M),), "ACG", [93, 94, 200])], None, dict(min_qual=0)))
    left = [rrec(b"ok", 0, 0, 0, 30, ((4, M),), "ACGT", 30), rrec(b"r1", -1, 0, 0, 30), rrec(b"r2", 2, 0, 0, 30), rrec(b"f4", 0, 0, 0x4, 30), rrec(b"f100", 0, 0, 0x100, 30),
            rrec(b"f200", 0, 0, 0x200, 30), rrec(b"f400", 0, 0, 0x400, 30), rrec(b"q0", 0, 0, 0, 0), rrec(b"q255", 0, 0, 0, 255), rrec(b"nq", 0, 0, 0, 30, qual=None),
            rrec(b"l0", 0, 0, 0, 30, ((3, N),), "", 30), rrec(b"no", 0, 0, 0, 30, (), "ACGT", 30), rrec(b"sup", 0, 0, 0x800, 30, ((4, M),), "ACGT", 30),
            rrec(b"f", 0, 0, 0x4, 30, ((9, M),), "ACGT", 30, b"XYZ")]
    out.append(("every reason a record is left out for", left, None, {}))
    for cap in (1, 2):
        out.append(("cap %d, both signs" % cap, [rrec(b"f", 0, 0, fl, 30, ((cap + 1, M),), "ACG"[:cap + 1], 30) for fl in (0, 0x91, 0x10)], None, dict(max_cycle=cap)))
    return out


def cut_record():
    """a counted record whose bytes do not hold the bases and qualities it announces: refused as not whole"""
    r = bytearray(rrec(b"cut", 0, 0, 0, 30, ((4, M),), "ACGT", 30))
    struct.pack_into("<I", r, 20, 40)
    return bytes(r)
