"""Host restatement of the device FASTA packer (csrc/fasta_pack.hip) in numpy, for cross-checking it.

What it restates: bns_fasta2bntseq + add1 over kseq_read in the reference (bwa_index/bntseq.c:233-330, kseq.h:95-215) --
the forward-only .pac, the .ann and the .amb that `bwa index` writes -- line by line with vectorised numpy, and glibc's
lrand48 after srand48(11) by jumping ahead through the affine map X -> a X + c (mod 2^48).
"""
from __future__ import annotations

import gzip

import numpy as np

LR_A, LR_C, LR_MASK = 0x5DEECE66D, 0xB, (1 << 48) - 1
LR_X0 = (11 << 16) | 0x330E

K_SEQ, K_HDR, K_EMPTY, K_PLUS = 0, 1, 2, 3

NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    NT4[_c] = _i
    NT4[_c + 32] = _i
NT4[ord("-")] = 5


def _jump_table():
    a, c, t = LR_A, LR_C, []
    for _ in range(48):
        t.append((a, c))
        c = (a * c + c) & LR_MASK
        a = (a * a) & LR_MASK
    return t


_JUMP = _jump_table()


def lrand48_states_at(k) -> np.ndarray:
    """the state X_{k+1} after the k-th draw (0-based) after srand48(11), for an array of k, by jump-ahead"""
    s = (np.asarray(k, dtype=np.uint64) + np.uint64(1)) & np.uint64(LR_MASK)
    x = np.full(s.shape, LR_X0, dtype=np.uint64)
    m = np.uint64(LR_MASK)
    with np.errstate(over="ignore"):
        for j, (a, c) in enumerate(_JUMP):
            bit = ((s >> np.uint64(j)) & np.uint64(1)).astype(bool)
            if bit.any():
                x = np.where(bit, (np.uint64(a) * x + np.uint64(c)) & m, x)
    return x


def lrand48_at(k) -> np.ndarray:
    """lrand48() of the k-th draw (0-based) after srand48(11): X_{k+1} >> 17"""
    return (lrand48_states_at(k) >> np.uint64(17)).astype(np.int64)


def lrand48_first(n: int) -> np.ndarray:
    """the first n draws of lrand48() after srand48(11), by doubling the computed prefix with jumps of its own length"""
    x = np.array([(LR_A * LR_X0 + LR_C) & LR_MASK], dtype=np.uint64)
    a, c = LR_A, LR_C                               # the map of len(x) steps
    m = np.uint64(LR_MASK)
    with np.errstate(over="ignore"):
        while x.size < n:
            x = np.concatenate([x, (np.uint64(a) * x + np.uint64(c)) & m])
            a, c = (a * a) & LR_MASK, (a * c + c) & LR_MASK
    return (x[:n] >> np.uint64(17)).astype(np.int64)


def lrand48_closed_form(k: int) -> int:
    """X_{k+1} >> 17 from X_j = a^j X_0 + c (a^j - 1) / (a - 1) (mod 2^48), in exact integers"""
    j = k + 1
    M = (1 << 48) * (LR_A - 1)
    aj = pow(LR_A, j, M)
    geo = (aj - 1) // (LR_A - 1)
    return (((aj % (1 << 48)) * LR_X0 + LR_C * geo) & LR_MASK) >> 17


def _isspace(c: int) -> bool:
    return c == 32 or 9 <= c <= 13


def _header(text: bytes):
    i = 0
    while i < len(text) and not _isspace(text[i]):
        i += 1
    name, comment = text[:i], b""
    if i < len(text):
        comment = text[i + 1:]
        if len(comment) > 1 and comment[-1:] == b"\r":
            comment = comment[:-1]
    return name, comment


def pack_fasta(data: bytes) -> dict:
    """what bns_fasta2bntseq(for_only=1) makes of the file's bytes: the kept text, the fill, the tables and the three files"""
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    b = np.frombuffer(data, np.uint8)
    n = b.size
    mk = np.flatnonzero((b == ord(">")) | (b == ord("@")))
    if mk.size == 0:
        raise ValueError("no FASTA record")
    start = int(mk[0])
    nl = np.flatnonzero(b == 10)
    nl = nl[nl >= start]
    ls = np.concatenate([[start], nl + 1]).astype(np.int64)
    ls = ls[ls < n]
    le = np.concatenate([ls[1:] - 1, [n - 1 if b[n - 1] == 10 else n]]).astype(np.int64)     # the line's '\n', or the file's end
    has_nl = le < n
    first = b[ls]
    kind = np.full(ls.size, K_SEQ, np.int8)
    kind[(first == ord(">")) | (first == ord("@"))] = K_HDR
    kind[first == ord("+")] = K_PLUS
    kind[first == 10] = K_EMPTY
    kind[0] = K_HDR
    if (kind == K_PLUS).any():
        raise ValueError("FASTQ")
    hdr = np.flatnonzero(kind == K_HDR)
    rec = np.cumsum(kind == K_HDR) - 1                                # record of every line
    seq = kind == K_SEQ
    cs = np.cumsum(seq)
    ordinal = cs - np.concatenate([[0], cs[hdr[1:] - 1]])[rec] if hdr.size else cs
    k = np.where(seq, le - ls, 0)
    last = np.maximum(le - 1, 0)
    cand = seq & (b[last] == 13)
    lone = k == 1
    trim = cand & np.where(has_nl, ~(lone & (ordinal == 1)), ~lone)
    k = k - trim
    # records
    recs = []
    for j in hdr:
        text = data[ls[j] + 1:le[j]]
        if not has_nl[j] and len(text) == 0:
            continue                                                  # a '>' as the file's last byte: no record
        recs.append(_header(text))
    n_rec_lines = hdr.size
    # kept bytes: every sequence line's first k bytes
    keep = np.zeros(n + 1, np.int64)
    np.add.at(keep, ls[k > 0], 1)
    np.add.at(keep, (ls + k)[k > 0], -1)
    keep = np.cumsum(keep[:n]) > 0
    T = b[keep]
    rec_of_byte = np.repeat(rec, k)
    rec_len = np.bincount(rec_of_byte, minlength=n_rec_lines)[:n_rec_lines]
    if len(recs) < n_rec_lines:                                       # the dropped record holds nothing
        rec_len = rec_len[:len(recs)]
    if not recs:
        raise ValueError("no FASTA record")
    if T.size == 0:
        raise ValueError("every sequence is empty")
    if ((T == 0) | (T >= 128)).any():
        raise ValueError("sequence byte 0 or >= 128")
    offsets = np.concatenate([[0], np.cumsum(rec_len)[:-1]]).astype(np.int64)
    recfirst = np.zeros(T.size, bool)
    recfirst[offsets[rec_len > 0]] = True
    c = NT4[T].astype(np.int64)
    amb = c >= 4
    prev = np.concatenate([[0], T[:-1]]).astype(np.int64)
    prev[recfirst] = 0
    hole = amb & (prev != T)
    rank = np.cumsum(amb) - 1
    n_amb = int(amb.sum())
    hole_off = np.flatnonzero(hole).astype(np.int64)
    hr = rank[hole_off]
    hole_len = np.diff(np.concatenate([hr, [n_amb]])).astype(np.int64)
    hole_char = T[hole_off]
    ends = offsets + rec_len
    n_ambs = np.bincount(np.searchsorted(ends, hole_off, side="right"), minlength=len(recs))[:len(recs)]
    codes = c.copy()
    codes[amb] = lrand48_first(n_amb) & 3
    l_pac = int(T.size)
    pad = np.concatenate([codes, np.zeros((-l_pac) % 4, np.int64)]).reshape(-1, 4)
    pac = ((pad[:, 0] << 6) | (pad[:, 1] << 4) | (pad[:, 2] << 2) | pad[:, 3]).astype(np.uint8)
    pac_file = pac.tobytes() + (b"\x00" if l_pac % 4 == 0 else b"") + bytes([l_pac % 4])
    ann = [b"%d %d 11\n" % (l_pac, len(recs))]
    for (name, comment), off, ln, na in zip(recs, offsets, rec_len, n_ambs):
        anno = comment.split(b"\0")[0] if comment else b"(null)"
        ann.append(b"0 " + name.split(b"\0")[0] + ((b" " + anno) if anno else b"") + b"\n")
        ann.append(b"%d %d %d\n" % (off, ln, na))
    amb_f = [b"%d %d %d\n" % (l_pac, len(recs), hole_off.size)]
    for o, ln, ch in zip(hole_off, hole_len, hole_char):
        amb_f.append(b"%d %d " % (o, ln) + bytes([ch]) + b"\n")
    return dict(text=T, codes=codes.astype(np.uint8), pac=pac, l_pac=l_pac, n_ambig=n_amb,
                names=[r[0] for r in recs], comments=[r[1] for r in recs], offsets=offsets, lens=rec_len.astype(np.int64),
                n_ambs=n_ambs.astype(np.int32), hole_off=hole_off, hole_len=hole_len, hole_char=hole_char,
                files={".pac": pac_file, ".ann": b"".join(ann), ".amb": b"".join(amb_f)})
