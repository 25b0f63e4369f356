"""Hand-made DEFLATE members for the one-lane inflater (csrc/inflate_core.h) at the limits the natural corpus of tests/test_inflate.py does not reach: codes of
every length 1 .. 15 on both alphabets (the lookup table ends at 9 bits, the canonical walk goes on to 15), a code-length code of 7 bits with the run symbols
at both ends of their repeats, runs over the literal / distance boundary and up to the last length, ndist 1, tokens of 48 bits at every bit offset, and the
refusals that need a hand-made header.  Written with test_inflate's BitWriter; what is expected of each member is zlib's own verdict (zlib_verdict)."""
import zlib

import numpy as np

from test_inflate import ECODES, ESYMBOL, OK, BitWriter, zlib_verdict

ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FLAT16 = [4] * 16 + [0, 0, 0]                       # a code-length code without run symbols: the lengths 0 .. 15, four bits each
LADDER = list(range(1, 16)) + [15]                  # 16 lengths, one of every length 1 .. 14 and two of 15: a complete code


def canon(lens) -> dict:
    """symbol -> (code, bits) of the canonical code of RFC 1951 3.2.2"""
    out, code = {}, 0
    for l in range(1, 16):
        for s, x in enumerate(lens):
            if x == l:
                out[s] = (code, l); code += 1
        code <<= 1
    return out


def expand(ops) -> list:
    out = []
    for op in ops:
        if isinstance(op, tuple):
            out += [out[-1] if op[0] == 16 else 0] * op[1]
        else:
            out.append(op)
    return out


def header(w: BitWriter, ops, cllen, nlen, ndist, last=1):
    """BFINAL, BTYPE 2 and the code lengths: ops are lengths 0 .. 15 or (16 | 17 | 18, repeats)"""
    ncode = max(i + 1 for i in range(19) if cllen[ORDER[i]] or i < 4)
    w.bits(last, 1); w.bits(2, 2); w.bits(nlen - 257, 5); w.bits(ndist - 1, 5); w.bits(ncode - 4, 4)
    for i in range(ncode):
        w.bits(cllen[ORDER[i]], 3)
    cc = canon(cllen)
    for op in ops:
        sym = op[0] if isinstance(op, tuple) else op
        w.code(*cc[sym])
        if sym == 16: w.bits(op[1] - 3, 2)
        elif sym == 17: w.bits(op[1] - 3, 3)
        elif sym == 18: w.bits(op[1] - 11, 7)


def zeros(n) -> list:
    """n zero lengths written one by one"""
    return [0] * n


def stored(w: BitWriter, data: bytes):
    w.bits(0, 1); w.bits(0, 2); w.align(); w.bits(len(data), 16); w.bits(len(data) ^ 0xFFFF, 16)
    w.out += data


def members() -> list:
    """(name, deflate data, isize, crc32, status).  Where zlib takes the member, isize and crc32 are its text's and the status is OK; the refusals carry the
    status csrc/inflate_core.h documents for them, and zlib refuses them too."""
    out = []

    def add(name, w, status=OK):
        data = w.done()
        d = zlib.decompressobj(-15)
        try:
            text = d.decompress(data)
            assert d.eof
        except (zlib.error, AssertionError):
            text = None
        assert (text is None) == (status != OK), name
        out.append((name, data, len(text) if text else 7, zlib.crc32(text) if text else 0, status))
        return text
    rnd = np.random.default_rng(12).integers(0, 256, 32768, dtype=np.uint8).tobytes()

    # literal codes of every length 1 .. 15: 'A' .. 'O' and the end-of-block code; no distance code at all (ndist 1, its length zero)
    llen = [0] * 257
    for i in range(15):
        llen[65 + i] = i + 1
    llen[256] = 15
    lc = canon(llen)
    w = BitWriter(); header(w, llen + [0], FLAT16, 257, 1)
    for s in list(range(65, 80)) + [74, 73, 256]:                # (lengths 9 and 10: either side of the lookup table, once more)
        w.code(*lc[s])
    assert add("literal codes of every length 1 .. 15", w) == b"ABCDEFGHIJKLMNOJI"

    # distance codes of every length 1 .. 15 on the symbols 14 .. 29, each with its largest extra field, behind 32 768 stored bytes
    dlen = [0] * 14 + LADDER
    dc = canon(dlen)
    w = BitWriter(); stored(w, rnd)
    l2 = [0] * 256 + [1, 1]
    header(w, l2 + dlen, FLAT16, 258, 30)
    for s in range(14, 30):
        w.code(*canon(l2)[257]); w.code(*dc[s]); w.bits((1 << DIST_EXTRA[s]) - 1, DIST_EXTRA[s])
    w.code(*canon(l2)[256])
    text = add("distance codes of every length 1 .. 15, the largest extra fields", w)
    assert len(text) == 32768 + 48 and text[-3:] == text[45:48]                  # (the last: distance 32 768)

    # a code-length code of 1 .. 7 bits over 0, 1, 3, 6, 8 and the run symbols; 16 with 3 and 6, 17 with 3 and 10, 18 with 11 and 138 repeats
    cl7 = [0] * 19
    for s, l in ((16, 1), (18, 2), (17, 3), (6, 4), (3, 5), (1, 6), (8, 7), (0, 7)):
        cl7[s] = l
    ops = [8, (16, 6), (16, 3), (18, 138), (18, 11), (17, 10), (17, 3), 1, 3, 6, 8] + [(16, 6)] * 13 + [(16, 3), 0]
    lens = expand(ops)
    assert len(lens) == 258 and max(cl7) == 7
    lc = canon(lens[:257])
    w = BitWriter(); header(w, ops, cl7, 257, 1)
    for s in (0, 9, 172, 173, 174, 200, 255, 256):
        w.code(*lc[s])
    assert add("a code-length code of 7 bits, the run symbols at both ends of their repeats", w) == bytes([0, 9, 172, 173, 174, 200, 255])

    # a run of 16 over the last literal / length lengths and the distance lengths, which ends at nlen + ndist
    cl = [0] * 19
    for s, l in ((0, 2), (1, 2), (2, 2), (16, 3), (18, 3)):
        cl[s] = l
    ops = zeros(97) + [1] + [(18, 138), (18, 19)] + [2, (16, 5)]
    lens = expand(ops)
    assert len(lens) == 261 and lens[255:] == [2] * 6
    lc, dc = canon(lens[:257]), canon(lens[257:])
    w = BitWriter(); header(w, ops, cl, 257, 4)
    for s in (97, 255, 97, 256):
        w.code(*lc[s])
    assert add("a run of 16 from the literal / length lengths into the distance lengths, up to the last", w) == b"a\xffa"
    # a run of 18 that is all 30 distance lengths and ends with them
    ops = zeros(97) + [1] + [(18, 138), (18, 20)] + [1, (18, 30)]
    assert len(expand(ops)) == 287
    lc = canon(expand(ops)[:257])
    w = BitWriter(); header(w, ops, cl, 257, 30)
    for s in (97, 97, 256):
        w.code(*lc[s])
    assert add("a run of 18 over all 30 distance lengths, every one zero", w) == b"aa"

    # ndist 1
    l3 = zeros(97) + [1] + zeros(158) + [2, 2]                     # 'a', the end-of-block code, length 3
    lc = canon(l3)
    for name, bit, status in (("ndist 1: one distance code of one bit, used", 0, OK), ("ndist 1: the unused half of the one-bit code", 1, ESYMBOL)):
        w = BitWriter(); header(w, l3 + [1], FLAT16, 258, 1)
        w.code(*lc[97]); w.code(*lc[257]); w.bits(bit, 1); w.code(*lc[256])
        assert add(name, w, status) == (b"aaaa" if status == OK else None)
    w = BitWriter(); header(w, l3 + [0], FLAT16, 258, 1)
    w.code(*lc[97]); w.code(*lc[97]); w.code(*lc[256])
    assert add("ndist 1: no distance code, literals only", w) == b"aa"

    # 48 bits: length symbol 284 behind 15 bits with 5 more, distance symbol 29 behind 15 bits with 13 more; k one-bit literals in front move it bit by bit
    llen = [0] * 285
    for i in range(14):
        llen[97 + i] = i + 1
    llen[256], llen[284] = 15, 15
    lc, dc = canon(llen), canon(dlen)
    for k in range(8):
        w = BitWriter(); stored(w, rnd)
        header(w, llen + dlen, FLAT16, 285, 30)
        for _ in range(k):
            w.code(*lc[97])
        at = len(w.out) * 8 + w.n
        w.code(*lc[284]); w.bits(30, 5); w.code(*dc[29]); w.bits(8191, 13)
        w.code(*lc[256])
        text = add(f"a token of 48 bits at bit offset {at % 8}", w)
        assert text == rnd + b"a" * k + (rnd + b"a" * k)[k:k + 257] and lc[284][1] == dc[29][1] == 15
    assert {int(m[0][-1]) for m in out[-8:]} == set(range(8))

    # refusals
    cl = [0] * 19
    for s, l in ((0, 1), (1, 2), (16, 2)):
        cl[s] = l
    w = BitWriter(); header(w, [], cl, 257, 1)
    w.code(*canon(cl)[16]); w.bits(0, 2); w.bits(0, 32)
    add("a repeat with no length before it", w, ECODES)
    cl = [0] * 19
    for s, l in ((0, 2), (1, 2), (2, 2), (16, 3), (18, 3)):
        cl[s] = l
    w = BitWriter(); header(w, zeros(97) + [1] + [(18, 138), (18, 20)] + [1, (18, 31)], cl, 257, 30); w.bits(0, 32)
    add("a repeat beyond the set", w, ECODES)
    w = BitWriter(); header(w, [], FLAT16, 287, 1); w.bits(0, 64)
    add("nlen 287", w, ECODES)
    w = BitWriter(); header(w, [], FLAT16, 257, 31); w.bits(0, 64)
    add("ndist 31", w, ECODES)
    for name, data, isize, crc, status in out:
        assert (zlib_verdict(data, isize, crc) is not None) == (status == OK), name
    return out
