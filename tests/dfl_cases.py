"""Hand-made pieces for the one-wave DEFLATE compressor (csrc/deflate_core.h): every structural limit of the Huffman builder, the bit writer, the 64-position
tokenizer, the position table and the stored / dynamic decision, each reached on purpose.  Plain numpy and zlib, no tests, no GPU.

Three tools, none of which shares code with the compressor:
  read_member   a Python inflater for one member that records the three code-length arrays, nlen / ndist / ncode and every token with its bit offset
                (counted from the member's first byte, as the compressor's 32-bit output words are) and its bits
  model_tokens  the tokenizer restated from the header comment of csrc/deflate_core.h: 64 positions a step, the position table read as it was before the
                step, hash (u32le * 2654435761) >> 19, the highest position wins a slot, a greedy walk with its carry, a step inside a match inserts nothing
  huff          the depth and cost of an unrestricted Huffman code of a histogram (heapq; among equal weights the shallower subtree first)

A case is a name, its data (one piece of at most 0xff00 bytes unless it says otherwise) and `must`: name -> predicate over evaluate()'s result, what the case
is about, checked on what the member holds and not on what the builder hoped.  A builder that stops reaching its edge fails the test that checks `must`."""
from __future__ import annotations

import bisect
import functools
import heapq
import struct
import zlib
from types import SimpleNamespace

import numpy as np

PIECE = 0xff00
STEP, MIN_MATCH, MAX_MATCH, MAX_DIST, HBITS = 64, 4, 258, 32768, 13
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
LEN_TOP = tuple(min(LEN_BASE[s] + (1 << LEN_EXTRA[s]) - 1, 257) for s in range(28)) + (258,)         # (symbol 284 ends at 257: 258 is symbol 285's)
DIST_TOP = tuple(DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1 for s in range(30))


def len_sym(length):
    return 285 if length == 258 else 257 + max(s for s in range(28) if LEN_BASE[s] <= length)


def dist_sym(dist):
    return max(s for s in range(30) if DIST_BASE[s] <= dist)


# ---------------------------------------------------------------------------------------------------------------- the token reader

def split_members(blob: bytes) -> list:
    out, p = [], 0
    while p < len(blob):
        assert blob[p:p + 4] == b"\x1f\x8b\x08\x04" and blob[p + 10:p + 16] == b"\x06\x00BC\x02\x00", p
        bs = struct.unpack_from("<H", blob, p + 16)[0] + 1
        out.append(blob[p:p + bs]); p += bs
    assert p == len(blob)
    return out


def _table(lens, maxbits):
    """peek of maxbits bits (the stream's order) -> (symbol, length) of the canonical code of RFC 1951 3.2.2, None where the bits are no code"""
    cnt = [0] * (maxbits + 2)
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, c = [0] * (maxbits + 2), 0
    for l in range(1, maxbits + 1):
        c = (c + cnt[l - 1]) << 1; nxt[l] = c
    tab = [None] * (1 << maxbits)
    for s, l in enumerate(lens):
        if l:
            v = nxt[l]; nxt[l] += 1
            r = int(format(v, "0%db" % l)[::-1], 2)
            for j in range(r, 1 << maxbits, 1 << l):
                tab[j] = (s, l)
    return tab


def read_member(m: bytes) -> SimpleNamespace:
    """One BGZF member with one deflate block, stored or dynamic: form, text, crc32 / isize as written, and of a dynamic block llen[nlen], dlen[ndist],
    cllen[19] (by symbol), nlen, ndist, ncode, tokens: (bit offset, bits, a literal | (length, distance)), eob: (bit offset, bits), end: the bit behind it"""
    assert m[:4] == b"\x1f\x8b\x08\x04" and m[10:16] == b"\x06\x00BC\x02\x00" and struct.unpack_from("<H", m, 16)[0] + 1 == len(m)
    crc, isize = struct.unpack("<II", m[-8:])
    r = SimpleNamespace(member=m, crc32=crc, isize=isize, tokens=[], llen=[], dlen=[], cllen=[], nlen=0, ndist=0, ncode=0)
    pad = m + b"\0" * 8
    pos = 144

    def take(n):
        nonlocal pos
        v = (int.from_bytes(pad[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v
    assert take(1) == 1, "one block, the last"
    btype = take(2)
    if btype == 0:
        n, nn = struct.unpack_from("<HH", m, 19)
        assert n ^ 0xffff == nn and len(m) == n + 31 and m[18] == 1
        r.form, r.text, r.end = "stored", m[23:23 + n], 8 * (23 + n)
        return r
    assert btype == 2, btype
    r.form = "dynamic"
    r.nlen, r.ndist, r.ncode = take(5) + 257, take(5) + 1, take(4) + 4
    r.cllen = [0] * 19
    for i in range(r.ncode):
        r.cllen[CL_ORDER[i]] = take(3)
    cl = _table(r.cllen, 7)
    lens = []
    while len(lens) < r.nlen + r.ndist:
        s, l = cl[take(7)]; pos -= 7 - l
        assert s < 16, "the compressor writes no run symbols"
        lens.append(s)
    r.llen, r.dlen = lens[:r.nlen], lens[r.nlen:]
    r.body = pos
    lt, dt = _table(r.llen, 15), _table(r.dlen, 15)
    out = bytearray()
    while True:
        at = pos
        s, l = lt[take(15)]; pos -= 15 - l
        if s < 256:
            out.append(s); r.tokens.append((at, pos - at, s))
        elif s == 256:
            r.eob = (at, pos - at); break
        else:
            length = LEN_BASE[s - 257] + take(LEN_EXTRA[s - 257])
            d, l = dt[take(15)]; pos -= 15 - l
            dist = DIST_BASE[d] + take(DIST_EXTRA[d])
            assert dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
            r.tokens.append((at, pos - at, (length, dist)))
    r.end, r.text = pos, bytes(out)
    assert len(m) == (pos + 7) // 8 + 8 and not take(-pos % 8), "the trailer follows the block's last byte, the bits between are zero"
    return r


# ---------------------------------------------------------------------------------------------------------------- the tokenizer's model

def hashes(piece: bytes) -> np.ndarray:
    a = np.frombuffer(piece, np.uint8).astype(np.uint64)
    if len(a) < 4:
        return np.zeros(0, np.int64)
    u = a[:-3] | a[1:-2] << np.uint64(8) | a[2:-1] << np.uint64(16) | a[3:] << np.uint64(24)
    return (((u * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(32 - HBITS)).astype(np.int64)


def model_tokens(piece: bytes, trace=None) -> list:
    """the tokens of one piece: a literal | (length, distance); trace (a list) receives (position, token) of every walked position"""
    n, h = len(piece), hashes(piece).tolist()
    tab = [0] * (1 << HBITS)
    out, carry = [], 0
    for b in range(0, n, STEP):
        if carry >= STEP:
            carry -= STEP
            continue
        lim, q = min(STEP, n - b), carry
        while q < lim:
            p, tok = b + q, None
            if p + 4 <= n:
                c = tab[h[p]]
                if c and p - (c - 1) <= MAX_DIST:
                    cand, maxl, k = c - 1, min(n - p, MAX_MATCH), 0
                    while k < maxl and piece[cand + k] == piece[p + k]:
                        k += 1
                    if k >= MIN_MATCH:
                        tok = (k, p - cand)
            if tok is None:
                tok = piece[p]
            out.append(tok)
            if trace is not None:
                trace.append((p, tok))
            q += tok[0] if isinstance(tok, tuple) else 1
        for p in range(b, min(b + STEP, n - 3)):
            tab[h[p]] = p + 1
        carry = q - STEP if q >= STEP else 0
    return out


def histograms(tokens: list) -> tuple:
    """(literal / length counts [286] with the end-of-block code, distance counts [30], extra bits)"""
    lf, df, extra = [0] * 286, [0] * 30, 0
    for t in tokens:
        if isinstance(t, tuple):
            ls, ds = len_sym(t[0]), dist_sym(t[1])
            lf[ls] += 1; df[ds] += 1; extra += LEN_EXTRA[ls - 257] + DIST_EXTRA[ds]
        else:
            lf[t] += 1
    lf[256] = 1
    return lf, df, extra


# ---------------------------------------------------------------------------------------------------------------- Huffman: depth, cost, Kraft sum

def huff(hist) -> tuple:
    """(depth, cost) of an unrestricted Huffman code of the counts that are not zero: the longest code and the sum of count x length.  One symbol: (1, count)."""
    heap = [(c, 0) for c in hist if c]
    if len(heap) == 1:
        return 1, heap[0][0]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1], cost


def kraft(lens, maxbits) -> int:
    """the Kraft sum of the lengths in units of 2^-maxbits: a complete code gives 1 << maxbits"""
    return sum(1 << (maxbits - l) for l in lens if l)


# ---------------------------------------------------------------------------------------------------------------- a case, evaluated

def evaluate(data: bytes, blob: bytes) -> SimpleNamespace:
    """what the musts look at: per piece the member as read and the model's trace, and for a one-piece case the same names at the top"""
    ms = split_members(blob)
    pieces = [data[p:p + PIECE] for p in range(0, len(data), PIECE)]
    assert len(ms) == len(pieces)
    out = []
    for m, pc in zip(ms, pieces):
        r = read_member(m)
        r.piece, r.n, r.walk = pc, len(pc), []
        r.model = model_tokens(pc, r.walk)
        r.lits = [t[2] for t in r.tokens if not isinstance(t[2], tuple)]
        r.matches = [t[2] for t in r.tokens if isinstance(t[2], tuple)]
        r.at = {}
        p = 0
        for t in r.tokens:                                       # position -> token, of the member's own tokens
            r.at[p] = t[2]
            p += t[2][0] if isinstance(t[2], tuple) else 1
        r.starts = sorted(r.at)
        r.lsyms = {len_sym(l) for l, _ in r.matches}
        r.dsyms = {dist_sym(d) for _, d in r.matches}
        r.maxbits = max((t[1] for t in r.tokens), default=0)
        r.spills = [t for t in r.tokens if (t[0] & 31) + t[1] > 64]
        out.append(r)
    top = SimpleNamespace(**vars(out[0]))
    top.pieces = out
    return top


def lit_at(r, a, b):
    """positions a .. b - 1 are literal tokens of the member"""
    return all(not isinstance(r.at.get(p), tuple) and p in r.at for p in range(a, b))


Case = functools.partial(SimpleNamespace, level=1)


# ---------------------------------------------------------------------------------------------------------------- building blocks

def de_bruijn(k: int) -> list:
    """a cyclic sequence over k values in which every ordered pair occurs once (length k * k)"""
    a, seq = [0] * (2 * 2), []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]; db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j; db(t + 1, t)
    db(1, 1)
    return seq


def fib(n: int) -> list:
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def skewed_literals(n_fib: int, n_flat: int, total: int, seed: int, skip: int = 1) -> bytes:
    """A piece without a match whose literal histogram is a Fibonacci ladder: the even bytes take n_fib values with the counts 1, 2, 3, 5 .. (the last
    value takes what is left of total / 2), the odd bytes walk a de Bruijn sequence over n_flat other values, so no pair of neighbouring odd bytes and with
    it no 4-byte window occurs twice."""
    half = total // 2
    assert n_flat * n_flat >= half + 1 and n_fib + n_flat <= 256
    f = fib(n_fib + skip - 1)[skip:]                             # (the end-of-block code is the ladder's first 1; skip 2: a length symbol the second)
    assert sum(f) < half
    counts = f + [half - sum(f)]
    rng = np.random.default_rng(seed)
    vals = rng.permutation(256)
    even = np.repeat(vals[:n_fib], counts).astype(np.uint8)
    rng.shuffle(even)
    odd = vals[n_fib:n_fib + n_flat][np.array(de_bruijn(n_flat)[:half])].astype(np.uint8)
    out = np.empty(2 * half, np.uint8)
    out[0::2], out[1::2] = even, odd
    return out.tobytes()


def word_stream(seed: int, tail: int = 0, lo: int = 12, hi: int = 29, robin: int = 17) -> bytes:
    """A piece of 4-byte words in which every word but its first occurrence is one match of 4 bytes at a chosen distance, so that the distance symbols lo .. hi
    occur with the counts of a ladder 1, 1, 2, 4, 7 .. (each count above the sum of all below it by an eighth: the Huffman tree of the ladder is a chain, one
    level per symbol).  Distances begin at 65 (symbol 12): a nearer copy can lie in the step of its match and is not in the position table yet.
      symbols lo .. robin   g words in turn, in the orders A = 1 2 3 4 .. and B = 2 1 4 3 .. alternately: a word comes back after g - 1, g or g + 1 words, and
                            what follows it differs from what followed it last time in its first byte (first bytes differ inside a section), so the match ends
      the symbols above     one word put into that stream again and again at a fixed spacing (first bytes 230 .. 255)
    The position table has 8 192 slots for all the 4-byte windows of the piece: the words' other three bytes are drawn again until no word's slot is taken by
    another window between two of its occurrences.  tail: that many more words of their own follow both occurrences of symbol hi's word, a match of 4 + 4 tail bytes."""
    rng = np.random.default_rng(seed)
    syms = list(range(lo, hi + 1))
    c = [1, 1]
    while len(c) < len(syms):
        c.append(sum(c[:-1]) * 9 // 8 + 1)
    cnt = dict(zip(reversed(syms), c))
    words = []

    def new_word(first):
        words.append([first] + [int(x) for x in rng.integers(0, 256, 3)])
        return len(words) - 1
    base = []
    for s in range(lo, robin + 1):
        g = (3 * DIST_BASE[s] + DIST_TOP[s]) // 16 + 1
        a = [new_word(int(f)) for f in rng.permutation(230)[:g]]
        b = a[:]
        for i in range(0, g - 1, 2):
            b[i], b[i + 1] = b[i + 1], b[i]
        for r in range(-(-cnt[s] // g) + 1):
            base += b if r & 1 else a
    n_words = len(base) + sum(cnt[s] for s in range(robin + 1, hi + 1)) + 30
    put, firsts, far = {}, iter(rng.permutation(26) + 230), None
    for s in range(hi, robin, -1):
        gap, left, start = (DIST_BASE[s] + DIST_TOP[s]) // 8, cnt[s], 1
        while left:
            while True:
                pos = [start + k * gap for k in range(left + 1) if start + k * gap < n_words - 2]
                if len(pos) >= 2 and not any(p + d in put for p in pos for d in (-1, 0, 1)):
                    break
                start += 1
            w = new_word(int(next(firsts)))
            far = w if far is None else far
            put.update((p, w) for p in pos)
            left -= len(pos) - 1; start += 3
    extra = [new_word(int(f)) for f in rng.integers(0, 230, tail)]
    stream, bi = [], 0
    for f in range(len(base) + len(put) + 10):
        if f in put:
            stream.append(put[f])
            if put[f] == far:
                stream += extra
        elif bi < len(base):
            stream.append(base[bi]); bi += 1
    w8, stream = np.array(words, np.uint8), np.array(stream)
    al = np.arange(len(stream) - 1) * 4
    first = np.zeros(len(al), bool)
    first[np.unique(stream[:len(al)], return_index=True)[1]] = True

    def state():
        data = w8[stream].reshape(-1)
        a = data.astype(np.uint64)
        u = a[:-3] | a[1:-2] << np.uint64(8) | a[2:-1] << np.uint64(16) | a[3:] << np.uint64(24)
        h = hashes(data.tobytes())
        order = np.argsort(h, kind="stable")                      # by slot, then by position
        prev = np.full(len(h), -1)
        same = h[order[1:]] == h[order[:-1]]
        prev[order[1:][same]] = order[:-1][same]                  # the position that holds the slot when p looks it up
        fail = ~first & ((prev[al] < 0) | (u[np.maximum(prev[al], 0)] != u[al]))
        return data, np.unique(stream[:len(al)][fail])
    data, bad = state()
    while len(bad):
        for _ in range(50):
            w8[bad[0], 1:] = rng.integers(0, 256, 3)
            data, bad2 = state()
            if len(bad2) < len(bad):
                break
        else:
            raise AssertionError("no words whose slots survive")
        bad = bad2
    return data.tobytes()


def noise(n: int, seed: int, lo: int = 0, hi: int = 64) -> bytes:
    """bytes lo .. hi - 1 drawn evenly (64 values: six bits a byte, a dynamic block): in a few thousand of them no 4-byte window comes twice (the musts of the
    cases that lean on it check their literals)"""
    return np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


def mark(n: int, seed: int) -> bytes:
    """n bytes 200 .. 255, no two of them equal (n <= 56): what a case plants"""
    return (np.random.default_rng(seed).permutation(56)[:n] + 200).astype(np.uint8).tobytes()


def same_slot(window: bytes, seed: int) -> bytes:
    """another 4-byte window (bytes 200 .. 255) with the hash of `window`"""
    want = int(hashes(window)[0])
    c = np.random.default_rng(seed).integers(200, 256, (1 << 17, 4), dtype=np.uint8)
    for row in c[hashes_of_rows(c) == want]:
        if row.tobytes() != window:
            return row.tobytes()
    raise AssertionError("no second window")


def hashes_of_rows(c: np.ndarray) -> np.ndarray:
    u = c[:, 0].astype(np.uint64) | c[:, 1].astype(np.uint64) << np.uint64(8) | c[:, 2].astype(np.uint64) << np.uint64(16) | c[:, 3].astype(np.uint64) << np.uint64(24)
    return (((u * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(32 - HBITS)).astype(np.int64)


def is_match(r, p, length=None, dist=None):
    t = r.at.get(p)
    return isinstance(t, tuple) and (length is None or t[0] == length) and (dist is None or t[1] == dist)


def covered(r, p, dist):
    """position p lies in a match of that distance"""
    q = r.starts[bisect.bisect_right(r.starts, p) - 1]
    t = r.at[q]
    return isinstance(t, tuple) and p < q + t[0] and t[1] == dist


def earlier_copy(r, p, k=4):
    """the k bytes at p stand somewhere before p, within the farthest distance"""
    return r.piece[p:p + k] in r.piece[max(0, p - MAX_DIST):p + k - 1]


# ---------------------------------------------------------------------------------------------------------------- the cases

def _huffman_limits() -> list:
    def ladder(which, depth):
        def must(r):
            lens = r.llen if which == "lit" else r.dlen
            hist = histograms([t[2] for t in r.tokens])[0 if which == "lit" else 1]
            return huff(hist)[0] >= depth and max(lens) == 15 and kraft(lens, 15) == 1 << 15
        return must
    no_match = lambda r: r.form == "dynamic" and not r.matches
    a, b = skewed_literals(18, 120, 20000, 1), skewed_literals(21, 180, 64000, 1)
    out = [Case(name="lit15: a literal ladder of depth 16", data=a, must={"no match": no_match, "deeper than 15 bits, written with 15, complete": ladder("lit", 16),
                                                                          "the largest ncode: 19": lambda r: r.ncode == 19}),
           Case(name="lit15: a literal ladder of depth 18", data=b, must={"no match": no_match, "deeper than 15 bits, written with 15, complete": ladder("lit", 18)})]
    d = word_stream(1)
    out.append(Case(name="dist15: 18 distance symbols in a ladder of depth 16", data=d,
                    must={"16 distance symbols or more": lambda r: len(r.dsyms) >= 16, "deeper than 15 bits, written with 15, complete": ladder("dist", 16)}))

    def cl7(r):
        hist = [(r.llen + r.dlen).count(i) for i in range(16)]
        return r.form == "dynamic" and huff(hist)[0] > 7 and max(r.cllen) == 7 and kraft(r.cllen, 7) == 128
    out.append(Case(name="cl7: code lengths in a ladder of depth 8", data=skewed_literals(14, 90, 2000, 1), must={"deeper than 7 bits, written with 7, complete": cl7}))
    return out


def far_pattern(dist: int, pad: int) -> bytes:
    """pad random bytes, then 200 bytes of 128 .. 255 twice, `dist` apart, between and behind them random ACGT letters (at most 256 slots of the position table)"""
    rng = np.random.default_rng(5)
    pat = rng.integers(128, 256, 200, dtype=np.uint8).tobytes()
    fill = rng.choice(np.frombuffer(b"ACGT", np.uint8), 40000).tobytes()
    return noise(pad, 17, 0, 256) + pat + fill[:dist - 200] + pat + fill[dist:dist + 300]


def _bit_writer() -> list:
    """spill: the padding in front of the pattern moves every token's offset; 6 was found by trying 0 .. 31 (also 7, 10, 19, 22).
    tok48: 15 + 5 + 15 + 13 bits.  A literal ladder of depth 15 whose two lowest rungs are the end-of-block code and length symbol 282, in front of the
    dist15 stream with 40 more words behind both occurrences of symbol 29's word: one match of 164 bytes at distance 28 832."""
    t48 = skewed_literals(17, 120, 20000, 1, skip=2) + word_stream(1, tail=40)

    def tok48(r):
        return any(bits == 48 and 281 <= len_sym(t[0]) <= 284 and dist_sym(t[1]) >= 28 and r.llen[len_sym(t[0])] == 15 and r.dlen[dist_sym(t[1])] == 15
                   for _, bits, t in r.tokens if isinstance(t, tuple))
    return [Case(name="spill: a token over three words", data=far_pattern(32768, 6), must={"a token with (offset mod 32) + bits > 64": lambda r: len(r.spills) >= 1}),
            Case(name="tok48: the longest token", data=t48, must={"a token of 48 bits": tok48, "the longest token has 48 bits": lambda r: r.maxbits == 48,
                                                                   "which spills": lambda r: any(t[1] == 48 for t in r.spills)})]


def _lengths() -> list:
    """A source of 258 marked bytes, then its first L bytes again for every L, the longest first (so that the copy before is no shorter), each behind a byte
    of its own; and a source of 700 bytes twice for the run beyond 258."""
    ends = sorted({LEN_BASE[s] for s in range(29)} | set(LEN_TOP), reverse=True)
    assert ends[-1] == 3 and ends[0] == 258 and 227 in ends and 257 in ends
    rng = np.random.default_rng(1)
    src, run = rng.integers(128, 256, 258, dtype=np.uint8).tobytes(), rng.integers(128, 256, 700, dtype=np.uint8).tobytes()
    data, at = bytearray(run + b"\x00" + run + b"\x01" + src), {}
    for i, L in enumerate(ends):
        data += bytes([2 + i]); at[L] = len(data); data += src[:L]
    data += b"\x7f"
    p = len(run) + 1
    must = {"every length symbol at both ends of its range": lambda r: all(is_match(r, at[L], L) for L in ends if L >= 4) and {len_sym(L) for L in ends if L >= 4} == set(range(258, 286)),
            "a repeat of 3 bytes is three literals": lambda r: lit_at(r, at[3], at[3] + 3),
            "a run beyond 258 gives 258 and goes on": lambda r: is_match(r, p, 258, p) and is_match(r, p + 258, 258, p) and is_match(r, p + 516, 700 - 516, p)}
    return [Case(name="lengths: every length symbol at both ends", data=bytes(data), must=must)]


def plant_pairs(data: bytearray, ds, seed: int, lo: int, hi: int, distinct_heads: bool) -> dict:
    """For every distance d a word of 6 bytes lo .. hi - 1 at b - d and again at b, the first lane of a step (so the copy at b - d lies in an earlier step
    whatever d is); for d below 6 a run of period d up to b + 6.  Returns d -> b."""
    rng = np.random.default_rng(seed)
    n, occ, at = len(data), bytearray(len(data)), {}
    heads = iter(rng.permutation(hi - lo) + lo)
    for d in ds:
        for b in range(64 * (-(-d // 64) + 1), n - 64, 64):
            spans = [(b - d - 2, b + 8)] if d < 10 else [(b - d - 2, b - d + 8), (b - 2, b + 8)]
            if not any(any(occ[x:y]) for x, y in spans):
                break
        else:
            raise AssertionError("no room")
        for x, y in spans:
            occ[x:y] = b"\1" * (y - x)
        head = next(heads) if distinct_heads else int(rng.integers(lo, hi))
        w = np.r_[head, [x for x in rng.permutation(hi - lo) + lo if x != head][:5]].astype(np.uint8)
        if d < 6:
            data[b - d:b + 6] = (bytes(w[:d]) * 8)[:d + 6]
        else:
            data[b - d:b - d + 6] = bytes(w); data[b:b + 6] = bytes(w)
        at[d] = b
    return at


def _distances() -> list:
    """One piece of the letter z, which the tokenizer covers with matches whose steps insert little, and in it a pair of words for every distance (plant_pairs;
    no two words begin alike: the z before a word and its first byte match the z before no other word).  A match may begin in the z before the word, where
    the z before its first copy are the candidate: the must asks for a match of distance d over b."""
    ds = sorted({DIST_BASE[s] for s in range(30)} | set(DIST_TOP) | {32769}, reverse=True)
    data = bytearray(b"z" * PIECE)
    at = plant_pairs(data, ds, 8, 128, 256, True)
    end = max(at.values()) + 80
    must = {"every distance symbol at both ends of its range": lambda r: all(covered(r, at[d], d) for d in ds if d <= MAX_DIST) and {dist_sym(d) for d in ds if d <= MAX_DIST} == set(range(30)),
            "distance 32 769 is refused": lambda r: lit_at(r, at[32769], at[32769] + 2) and r.piece[at[32769] - 32769:][:6] == r.piece[at[32769]:][:6]}
    return [Case(name="distances: every distance symbol at both ends", data=bytes(data[:end]), must=must)]


def letters(n: int, seed: int) -> bytes:
    """text over twelve letters: 4-byte windows come back all the time"""
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGT\t\n012345", np.uint8), n).tobytes()


def _step_edges() -> list:
    """Sources of 10, 10, 68, 69 and 258 marked bytes in the first steps of 2 048 noise bytes, and their copies where the walk meets a step's edge.
    Bytes seen only inside a skipped step: W, 8 bytes of the 258-byte source whose copy lies in step 20, which that match covers whole; between the source and
    the copy stands another window with W's hash, which takes W's slot.  Were step 20 inserted, W at 1 500 would find its copy at 1 290; it finds the other window, and
    the seven bytes behind its first find the source at 385, not the copy at 1 291."""
    data = bytearray(noise(2048, 31))
    s1, s2, s3, s4, s5 = mark(10, 1), mark(10, 2), noise(68, 3, 200, 256), noise(69, 4, 200, 256), noise(258, 5, 200, 256)
    for at, src in ((2, s1), (14, s2), (64, s3), (140, s4), (256, s5), (630, s1), (695, s2), (828, s3), (1020, s4), (1162, s5)):
        data[at:at + len(src)] = src
    w = s5[128:136]
    other = same_slot(w[:4], 9)
    data[600:604] = other
    data[1500:1508] = w
    must = {"a match ends on a step's last byte": lambda r: is_match(r, 630, 10) and 640 in r.at,
            "a match ends one byte into the next step": lambda r: is_match(r, 695, 10) and 705 in r.at,
            "a carry of exactly 64: a whole step skipped, the next begins at lane 0": lambda r: is_match(r, 828, 68) and 896 in r.at,
            "a carry of 65": lambda r: is_match(r, 1020, 69) and 1089 in r.at,
            "a carry across four steps": lambda r: is_match(r, 1162, 258) and 1420 in r.at and 1420 // 64 - 1162 // 64 == 4,
            "bytes seen only inside a skipped step give literals": lambda r: lit_at(r, 1500, 1501) and is_match(r, 1501, 7, 1501 - 385) and r.piece[1290:1298] == w and 1290 // 64 * 64 > 1162 and earlier_copy(r, 1500, 8)
            and int(hashes(other)[0]) == int(hashes(w[:4])[0]) and other != w[:4]}
    return [Case(name="step edges", data=bytes(data), must=must)]


def _piece_edges() -> list:
    out = []
    for n in (1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, PIECE - 1, PIECE):
        out.append(Case(name=f"piece of {n} bytes", data=letters(n, n), must={"the member holds the piece": lambda r, n=n: r.n == n and r.text == r.piece and r.isize == n}))
    s = mark(12, 3)
    d = bytearray(noise(500, 42)); d[100:112] = s; d[-12:] = s
    out.append(Case(name="a match up to the last byte", data=bytes(d), must={"the last token is the match": lambda r: is_match(r, 488, 12, 388) and r.starts[-1] == 488}))
    d = bytearray(noise(300, 33)); d[100:108] = s[:8]; d[-3:] = s[:3]
    out.append(Case(name="a repeat in the last three positions", data=bytes(d), must={"three literals": lambda r: lit_at(r, 297, 300) and earlier_copy(r, 297, 3)}))
    d = bytearray(noise(300, 34)); d[0:8] = s[:8]; d[100:108] = s[:8]
    out.append(Case(name="a candidate at position 0", data=bytes(d), must={"a match whose distance is its position": lambda r: is_match(r, 100, 8, 100)}))
    d = noise(PIECE - 8, 35) + s[:8] + s[:8] + noise(3000, 36)
    out.append(Case(name="a repeat across two pieces of one call", data=d,
                    must={"two pieces": lambda r: len(r.pieces) == 2 and r.pieces[0].piece[-8:] == r.pieces[1].piece[:8],
                          "the second piece begins with literals": lambda r: lit_at(r.pieces[1], 0, 8)}))
    return out


def _hash_table() -> list:
    w = mark(4, 4)
    v = same_slot(w, 10)
    a, b, y = w + mark(4, 5), v + mark(4, 6), mark(8, 7)
    d = bytearray(noise(1100, 37))
    for at, x in ((5, a), (20, b), (131, b), (263, a), (400, y), (500, y), (600, y), (700, b[:4] + mark(4, 8)), (900, a[:4] + mark(4, 9))):
        d[at:at + len(x)] = x
    same = lambda r: int(hashes(w)[0]) == int(hashes(v)[0]) and w != v
    must = {"two lanes of one step with one hash: a later match names the higher": lambda r: same(r) and is_match(r, 131, 8, 111),
            "the lower lane's window finds the other in its slot: refused": lambda r: same(r) and lit_at(r, 263, 264) and is_match(r, 264, 7, 258) and earlier_copy(r, 263, 8),
            "the same window three times: the latest wins": lambda r: is_match(r, 500, 8, 100) and is_match(r, 600, 8, 100),
            "two windows with one hash, one after the other: refused both ways": lambda r: lit_at(r, 700, 704) and lit_at(r, 900, 904)}
    return [Case(name="hash table", data=bytes(d), must=must)]


def _small_codes() -> list:
    """ncode: the code-length code's lengths are written in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 up to the last that is in use.  The largest
    is 19 (a code of 15 bits: the ladders above).  The smallest: a complete distance code has a length of 4 or less (30 symbols of 5 bits and more fall
    short of a Kraft sum of one; the place-holders have 1), and 4 stands twelfth: 16 distance symbols once each, beside literals and lengths of 5 .. 11 bits."""
    out = [Case(name="no match: two place-holder distance codes", data=skewed_literals(10, 40, 1000, 2),
                must={"no match, distance symbols 0 and 1 of one bit, nlen 257": lambda r: r.form == "dynamic" and not r.matches and r.dlen == [1, 1] and r.nlen == 257}),
           Case(name="one distance symbol, symbol 0", data=b"a" * 200,
                must={"one match of distance 1, a place-holder beside it": lambda r: r.matches == [(136, 1)] and r.dlen == [1, 1]}),
           Case(name="nlen 286", data=b"a" * 400, must={"length 258 is in use": lambda r: (258, 1) in r.matches and r.nlen == 286 and r.llen[285] > 0})]
    fill = skewed_literals(12, 160, 24700, 4)
    x = mark(8, 21)                                               # (the 21st try: a word whose slot none of the 24 700 windows between takes)
    out.append(Case(name="one distance symbol, symbol 29", data=x + fill + x + mark(4, 12),
                    must={"one match, symbol 29 and the place-holder 0 of one bit, ndist 30": lambda r: len(r.matches) == 1 and r.dsyms == {29} and r.ndist == 30 and r.dlen[0] == r.dlen[29] == 1 and sum(r.dlen) == 2}))
    d = bytearray(noise(3000, 38, 0, 128))
    ds = [DIST_BASE[s] for s in range(6, 22)]
    at = plant_pairs(d, sorted(ds, reverse=True), 12, 0, 128, False)
    out.append(Case(name="the smallest ncode", data=bytes(d[:max(at.values()) + 200]),
                    must={"16 distance symbols of 4 bits, ncode 12": lambda r: all(covered(r, at[x], x) for x in ds) and [l for l in r.dlen if l] == [4] * 16 and r.ncode == 12}))
    return out


def _many_pieces() -> list:
    parts = []
    for i in range(40):
        parts.append((noise(PIECE, 100 + i, 0, 256), letters(PIECE, 100 + i), b"\0" * PIECE, (letters(211, i) * 400)[:PIECE], skewed_literals(21, 180, 64000, i) + b"q" * 1280)[i % 5])
    parts.append(b"!")

    def offsets(r):
        off = np.cumsum([0] + [len(x.member) for x in r.pieces[:-1]])
        return {int(o) % 4 for o in off} == {0, 1, 2, 3}
    must = {"41 pieces, the last of one byte": lambda r: len(r.pieces) == 41 and r.pieces[-1].n == 1,
            "stored, dynamic and tiny members": lambda r: {x.form for x in r.pieces} == {"stored", "dynamic"} and min(len(x.member) for x in r.pieces[:-1]) < 600,
            "members begin at every alignment": offsets}
    return [Case(name="one call of 41 pieces", data=b"".join(parts), must=must)]


def boundary_stream() -> bytes:
    """9 000 bytes, half of the values 2.08 times as frequent as the other half: a dynamic block saves about 0.16 bits a byte, and some 500 bits of header cost"""
    p = np.r_[np.full(128, 1.35), np.full(128, 0.65)]
    return np.random.default_rng(0).choice(256, 9000, p=p / p.sum()).astype(np.uint8).tobytes()


SMALLER, TIE = (6059, 6060, 6061, 6062, 6064), (6058, 6057, 6033, 6017)


def _form_decision() -> list:
    """Prefixes of boundary_stream(), found with the trace of tests/deflate_core_host.cpp by trying every length from 5 600 to 9 000: no match in any of them.
    SMALLER: the dynamic block has 8 n + 25 .. 8 n + 32 bits, the member n + 30 bytes, one fewer than stored; at 6 059 the bits are a multiple of eight, at 6 060,
    6 061 and 6 064 one short of it: two bits more (the two place-holder distance codes, which no token uses) and the estimate reaches the stored size.
    TIE: n + 31 bytes either way; stored is written.  test_dfl_cases.py checks those sizes from the trace, with the model's counts."""
    s = boundary_stream()
    out = [Case(name=f"form: dynamic is one byte smaller at {n}", data=s[:n], kind="smaller",
                must={"no match, dynamic, n + 30 bytes": lambda r: r.form == "dynamic" and not r.matches and len(r.member) == r.n + 30}) for n in SMALLER]
    out += [Case(name=f"form: a tie at {n}", data=s[:n], kind="tie", must={"stored": lambda r: r.form == "stored" and len(r.member) == r.n + 31}) for n in TIE]
    return out


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = _huffman_limits() + _bit_writer() + _lengths() + _distances() + _step_edges() + _piece_edges() + _hash_table() + _small_codes() + _form_decision() + _many_pieces()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def stored_member(piece: bytes) -> bytes:
    """the member of a piece in the stored form, from the gzip and BGZF specifications"""
    n = len(piece)
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", n + 30) + b"\x01" + struct.pack("<HH", n, n ^ 0xffff) + piece
            + struct.pack("<II", zlib.crc32(piece), n))


def dynamic_bits(llen, dlen, cllen, tokens) -> int:
    """the bits of the dynamic block of these tokens under these code lengths, from BFINAL to the end-of-block code, as RFC 1951 3.2.7 lays it out without
    run symbols"""
    lf, df, extra = histograms(tokens)
    nlen = max([257] + [i + 1 for i in range(len(llen)) if llen[i]])
    ndist = max([1] + [i + 1 for i in range(len(dlen)) if dlen[i]])
    ncode = max([4] + [i + 1 for i in range(19) if cllen[CL_ORDER[i]]])
    return (3 + 14 + 3 * ncode + sum(cllen[x] for x in llen[:nlen]) + sum(cllen[x] for x in dlen[:ndist])
            + sum(a * b for a, b in zip(lf, llen)) + sum(a * b for a, b in zip(df, dlen)) + extra)
