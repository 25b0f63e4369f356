"""The DEFLATE decoder of the device inflate (csrc/inflate_core.h) compiled as plain C++ under AddressSanitizer and UBSan (tests/inflate_core_host.cpp: every
member's input and output are heap blocks of exactly their sizes): a corpus of members written by zlib in every block form against zlib.decompress and
zlib.crc32, a few thousand damaged members against zlib's own verdict, hand-made members for every refusal, and the member-table scan (bmh_bgzf_scan).
The same corpus runs through the kernel in test_inflate_gpu.py."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from test_reads_input import FIX, FIXTURES, bgzf, fixture_text

HERE = os.path.dirname(os.path.abspath(__file__))
OK, EBTYPE, ESTORED, ECODES, ESYMBOL, EDIST, ETRUNC, ESIZE, ECRC, ETABLE = range(10)


# ---------------------------------------------------------------------------------------------------------------- the corpus

def raw(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_FULL_FLUSH) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, p = [], 0
    for q in list(flush_at) + [len(data)]:
        out.append(c.compress(data[p:q]))
        if q < len(data):
            out.append(c.flush(flush))
        p = q
    out.append(c.flush())
    return b"".join(out)


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):                  # a field: least significant bit first
        self.acc |= v << self.n; self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255); self.acc >>= 8; self.n -= 8

    def code(self, v, n):                  # a Huffman code: most significant bit first
        for k in range(n - 1, -1, -1):
            self.bits((v >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def fixed_sym(self, s):                # a literal / length symbol of the fixed code
        if s < 144: self.code(0x30 + s, 8)
        elif s < 256: self.code(0x190 + s - 144, 9)
        elif s < 280: self.code(s - 256, 7)
        else: self.code(0xC0 + s - 280, 8)

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


def synthetic_fastq(n_bytes: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    recs, size, i = [], 0, 0
    while size < n_bytes:
        ln = int(rng.integers(100, 152))
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), ln).tobytes()
        q = (rng.integers(0, 8, ln) * 5 + 35).astype(np.uint8).tobytes()
        r = b"@r%d/1 lane:%d\n%s\n+\n%s\n" % (i, i % 8, seq, q)
        recs.append(r); size += len(r); i += 1
    return b"".join(recs)


def far_copy_member() -> tuple:
    """32 768 random bytes in a stored block, then the same bytes again as matches at distance 32 768 (lengths 258, 257 and 3) in a fixed block"""
    rnd = np.random.default_rng(11).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = BitWriter()
    w.bits(0, 1); w.bits(0, 2); w.align(); w.bits(32768, 16); w.bits(32768 ^ 0xFFFF, 16)
    w.out += rnd
    w.bits(1, 1); w.bits(1, 2)

    def match(sym, extra_bits, extra):
        w.fixed_sym(sym)
        if extra_bits: w.bits(extra, extra_bits)
        w.code(29, 5); w.bits(32768 - 24577, 13)
    for _ in range(126): match(285, 0, 0)
    match(284, 5, 257 - 227); match(257, 0, 0)
    assert 126 * 258 + 257 + 3 == 32768
    w.fixed_sym(256)
    return rnd + rnd, w.done()


def corpus() -> list:
    """(name, text, raw deflate data)"""
    rng = np.random.default_rng(7)
    fq = synthetic_fastq(3 << 20, 1)
    piece = fq[:60000]
    out = []
    for lv in (0, 1, 6, 9):
        out.append((f"fastq level {lv}", piece, raw(piece, lv)))
    for name, st in (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huffman only", zlib.Z_HUFFMAN_ONLY), ("filtered", zlib.Z_FILTERED)):
        out.append((f"fastq {name}", piece, raw(piece, 6, st)))
    out.append(("full flush", piece, raw(piece, 6, flush_at=(1, 20000, 20000, 45000))))
    out.append(("sync flush", piece, raw(piece, 6, flush_at=(777, 30000), flush=zlib.Z_SYNC_FLUSH)))
    out.append(("sync flush, fixed", piece[:5000], raw(piece[:5000], 6, zlib.Z_FIXED, flush_at=(100, 100, 2500), flush=zlib.Z_SYNC_FLUSH)))
    out.append(("empty", b"", raw(b"")))
    out.append(("one byte", b"x", raw(b"x")))
    out.append(("65536 identical", b"A" * 65536, raw(b"A" * 65536, 9)))
    out.append(("65536 identical, stored", b"A" * 65536, raw(b"A" * 65536, 0)))
    out.append(("distance 32768",) + far_copy_member())
    near = rng.integers(0, 256, 32506, dtype=np.uint8).tobytes()
    out.append(("zlib's farthest distance", near + near, raw(near + near, 9)))
    rnd = rng.integers(0, 256, 65280, dtype=np.uint8).tobytes()
    out.append(("65280 random", rnd, raw(rnd)))
    out.append(("65280 random, level 0", rnd, raw(rnd, 0)))
    full = fq[100000:100000 + 65536]
    out.append(("exactly 65536", full, raw(full)))
    skew = bytes(rng.choice(np.arange(256, dtype=np.uint8), 40000, p=np.r_[[0.55, 0.25], np.full(254, 0.2 / 254)]))     # codes beyond 9 bits
    out.append(("skewed bytes", skew, raw(skew, 6, zlib.Z_HUFFMAN_ONLY)))
    for name in FIXTURES:
        t = fixture_text(name)
        for k in range(0, len(t), 777):
            out.append((f"{name}@{k}", t[k:k + 777], raw(t[k:k + 777])))
        out.append((name, t[:65536], raw(t[:65536])))
    for k in range(0, len(fq), 60000):
        out.append((f"synthetic@{k}", fq[k:k + 60000], raw(fq[k:k + 60000])))
    for name, text, data in out:
        assert zlib.decompress(data, -15) == text and len(text) <= 65536, name
    return out


def handmade() -> list:
    """(name, deflate data, isize, crc32, status): one member per refusal"""
    out = []
    w = BitWriter(); w.bits(1, 1); w.bits(1, 2); w.fixed_sym(ord("a")); w.fixed_sym(257); w.code(1, 5); w.fixed_sym(256)
    out.append(("distance beyond the start", w.done(), 4, 0, EDIST))
    w = BitWriter(); w.bits(1, 1); w.bits(3, 2)
    out.append(("block type 3", w.done(), 0, 0, EBTYPE))
    w = BitWriter(); w.bits(1, 1); w.bits(0, 2); w.align(); w.bits(5, 16); w.bits(5, 16); w.out += b"hello"
    out.append(("LEN / NLEN", w.done(), 5, zlib.crc32(b"hello"), ESTORED))
    w = BitWriter(); w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(0, 4)
    for _ in range(4): w.bits(1, 3)
    w.bits(0, 32)
    out.append(("over-subscribed code lengths", w.done(), 10, 0, ECODES))
    w = BitWriter(); w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(0, 4); w.bits(1, 3); w.bits(0, 9); w.bits(0, 32)
    out.append(("incomplete code lengths", w.done(), 10, 0, ECODES))
    # a complete code-length code {0: 1 bit, 8: 1 bit}; literals 0 and 1 with 8 bits each and nothing else: incomplete, and no end-of-block code
    w = BitWriter(); w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(1, 4); w.bits(0, 9); w.bits(1, 3); w.bits(1, 3)
    w.code(1, 1); w.code(1, 1)
    for _ in range(256): w.code(0, 1)
    w.bits(0, 32)
    out.append(("incomplete literal set", w.done(), 10, 0, ECODES))
    text = bytes(range(100))
    d = raw(text)
    out.append(("output beyond ISIZE", d, 50, zlib.crc32(text[:50]), ESIZE))
    out.append(("output short of ISIZE", d, 150, zlib.crc32(text), ESIZE))
    out.append(("ISIZE above 65536", d, 70000, zlib.crc32(text), ESIZE))
    out.append(("wrong CRC", d, 100, zlib.crc32(text) ^ 1, ECRC))
    out.append(("ends early", d[:-3], 100, zlib.crc32(text), ETRUNC))
    out.append(("no data", b"", 0, 0, ETRUNC))
    w = BitWriter(); w.bits(1, 1); w.bits(1, 2); w.fixed_sym(286); w.fixed_sym(256)
    out.append(("length symbol 286", w.done(), 0, 0, ESYMBOL))
    w = BitWriter(); w.bits(1, 1); w.bits(1, 2); w.fixed_sym(ord("a")); w.fixed_sym(257); w.code(30, 5); w.fixed_sym(256)
    out.append(("distance symbol 30", w.done(), 4, 0, ESYMBOL))
    return out


def damaged(members: list, n_cases: int, seed: int) -> list:
    """(name, data, isize, crc32): single-bit flips and truncations of the corpus's members"""
    rng = np.random.default_rng(seed)
    out = []
    small = [m for m in members if len(m[2]) > 0]
    while len(out) < n_cases:
        name, text, data = small[int(rng.integers(len(small)))]
        crc = zlib.crc32(text)
        if rng.random() < 0.75:
            # the block headers and code lengths are at the front: half the flips go there
            bit = int(rng.integers(min(len(data) * 8, 800))) if rng.random() < 0.5 else int(rng.integers(len(data) * 8))
            d = bytearray(data); d[bit >> 3] ^= 1 << (bit & 7)
            out.append((f"{name}: bit {bit}", bytes(d), len(text), crc))
        else:
            cut = int(rng.integers(len(data)))
            out.append((f"{name}: cut at {cut}", data[:cut], len(text), crc))
    return out


def zlib_verdict(data: bytes, isize: int, crc: int):
    """the text when zlib inflates the member to isize bytes with that CRC32 (what the host inflate accepts), else None"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(data, 65537)
    except zlib.error:
        return None
    if not d.eof or len(text) != isize or zlib.crc32(text) != crc:
        return None
    return text


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

@pytest.fixture(scope="module")
def core_exe():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "inflate_core_host")
    src = [os.path.join(HERE, "inflate_core_host.cpp"), os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc", "inflate_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def run_core(exe, tmp_path, cases: list) -> list:
    """cases: (data, isize, crc32) -> (status, bytes produced, crc32 of them, the text when the status is 0)"""
    fi, fo = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for data, isize, crc in cases:
            f.write(struct.pack("<III", len(data), isize, crc & 0xFFFFFFFF) + data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:verify_asan_link_order=0")
    r = subprocess.run([exe, fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    with open(fo, "rb") as f:
        blob = f.read()
    out, p = [], 0
    for _ in cases:
        st, got, crc = struct.unpack_from("<III", blob, p); p += 12
        text = None
        if st == 0:
            text = blob[p:p + got]; p += got
        out.append((st, got, crc, text))
    assert p == len(blob)
    return out


def test_corpus_equals_zlib(core_exe, tmp_path):
    members = corpus()
    res = run_core(core_exe, tmp_path, [(data, len(text), zlib.crc32(text)) for _, text, data in members])
    for (name, text, data), (st, got, crc, out) in zip(members, res):
        assert st == OK and got == len(text), (name, st, got)
        assert out == text == zlib.decompress(data, -15), name
        assert crc == zlib.crc32(text), name


def test_handmade_refusals(core_exe, tmp_path):
    cases = handmade()
    res = run_core(core_exe, tmp_path, [(d, isize, crc) for _, d, isize, crc, _ in cases])
    for (name, d, isize, crc, want), (st, got, _, _) in zip(cases, res):
        assert st == want, (name, st, want)
        assert got <= min(isize, 65536), name
        assert zlib_verdict(d, isize, crc) is None, name


def test_limit_members(core_exe, tmp_path):
    """tests/inflate_limits.py: codes of 1 .. 15 bits on both alphabets, the 7-bit code-length code, runs over the literal / distance boundary, ndist 1, tokens of
    48 bits at every bit offset: OK exactly where zlib takes the member, with zlib's text; the refusals with the status the core documents"""
    import inflate_limits
    cases = inflate_limits.members()
    assert len(cases) == 20 and sum(st == OK for *_, st in cases) == 15
    res = run_core(core_exe, tmp_path, [(d, isize, crc) for _, d, isize, crc, _ in cases])
    for (name, d, isize, crc, want), (st, got, crc_got, out) in zip(cases, res):
        text = zlib_verdict(d, isize, crc)
        assert (st == OK) == (text is not None) and st == want, (name, st, want)
        if text is not None:
            assert out == text == zlib.decompress(d, -15) and got == isize and crc_got == crc, name
        else:
            assert got <= min(isize, 65536), name


def test_damaged_members_end_with_a_status(core_exe, tmp_path):
    """4000 single-bit flips and truncations: no sanitizer report; the member is refused unless zlib inflates it to the same size and CRC32, and then the bytes are zlib's"""
    cases = damaged(corpus(), 4000, seed=3)
    res = run_core(core_exe, tmp_path, [(d, isize, crc) for _, d, isize, crc in cases])
    n_ok = 0
    seen = set()
    for (name, d, isize, crc), (st, got, _, out) in zip(cases, res):
        want = zlib_verdict(d, isize, crc)
        assert got <= min(isize, 65536), name
        if want is None:
            assert st != OK, name
        else:
            assert st == OK and out == want, name
            n_ok += 1
        seen.add(st)
    # the set is not all of one kind: most refusals occur in it
    assert {ETRUNC, ECRC, ESIZE, ECODES, EDIST} <= seen, seen
    assert n_ok < len(cases) // 4


# ---------------------------------------------------------------------------------------------------------------- the library: host mode and the member table

def test_library_host_mode_equals_zlib():
    from bwamem_hip.lib import bgzf_scan, inflate_bgzf, inflate_members
    fq = synthetic_fastq(1 << 20, 5)
    for block in (777, 60000, 65280):
        z = bgzf(fq, block)
        assert inflate_bgzf(z, host=True) == fq
        tab, used, text = bgzf_scan(z)
        assert used == len(z) and text == len(fq) and len(tab) == -(-len(fq) // block) + 1
        assert tab["isize"][-1] == 0 and np.array_equal(tab["out_off"], np.concatenate([[0], np.cumsum(tab["isize"])[:-1]]))
        out, st = inflate_members(z, tab, text, host=True)
        assert not st.any() and out.tobytes() == fq
    assert inflate_bgzf(b"", host=True) == b""
    z = bytearray(bgzf(fq[:200000], 60000)); z[len(z) // 2] ^= 0x10
    with pytest.raises(ValueError, match=r"damaged BGZF member 1 \("):
        inflate_bgzf(bytes(z), host=True)
    with pytest.raises(ValueError, match="truncated"):
        inflate_bgzf(bgzf(fq[:200000], 60000)[:-40], host=True)
    # table entries that point outside the buffers are refused per member, not followed
    tab, used, text = bgzf_scan(bgzf(fq[:5000], 777))
    bad = tab.copy(); bad["in_off"][1] = 1 << 40; bad["out_off"][2] = text; bad["in_len"][3] = 1 << 31
    out, st = inflate_members(bgzf(fq[:5000], 777), bad, text, host=True)
    assert list(st[:5]) == [OK, ETABLE, ETABLE, ETABLE, OK]


def _member(text: bytes, extra_before: bytes = b"", extra_after: bytes = b"", bc: bool = True) -> bytes:
    z = raw(text)
    xlen = len(extra_before) + (6 if bc else 0) + len(extra_after)
    size = 12 + xlen + len(z) + 8
    extra = extra_before + (b"BC\x02\x00" + struct.pack("<H", size - 1) if bc else b"") + extra_after
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra + z + struct.pack("<II", zlib.crc32(text), len(text))


def test_member_table_scan():
    from bwamem_hip.lib import bgzf_scan, inflate_bgzf
    xy = b"XY\x03\x00abc"
    a, b, c = _member(b"first\n", extra_before=xy), _member(b"second\n", extra_after=xy), _member(b"third\n", extra_before=xy + b"ZZ\x00\x00")
    tab, used, text = bgzf_scan(a + b + c)
    assert len(tab) == 3 and used == len(a + b + c) and text == 19
    assert list(tab["in_off"]) == [12 + 13, len(a) + 12 + 13, len(a + b) + 12 + 17] and list(tab["isize"]) == [6, 7, 6]
    assert list(tab["crc32"]) == [zlib.crc32(b"first\n"), zlib.crc32(b"second\n"), zlib.crc32(b"third\n")]
    assert list(tab["in_len"]) == [len(raw(t)) for t in (b"first\n", b"second\n", b"third\n")]
    assert inflate_bgzf(a + b + c, host=True) == b"first\nsecond\nthird\n"
    # a cut header and a cut body: the members before them, and where they end
    for cut in (len(a) + 5, len(a) + 14, len(a) + len(b) - 1):
        tab, used, text = bgzf_scan((a + b + c)[:cut])
        assert len(tab) == 1 and used == len(a) and text == 6, cut
    # a member without BC (a plain gzip member with another extra field) is no BGZF member
    with pytest.raises(ValueError, match=rf"bytes at {len(a)} begin no BGZF member"):
        bgzf_scan(a + _member(b"x", extra_before=xy, bc=False) + c)
    with pytest.raises(ValueError, match="bytes at 0 begin no BGZF member"):
        bgzf_scan(b"@r1\nACGT\n+\nIIII\n")
