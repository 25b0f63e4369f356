"""The BAM output's two cores as plain C++ under AddressSanitizer and UBSan (tests/bam_core_host.cpp, tests/deflate_core_host.cpp) and through the library's
host entry points: SAM lines -> BAM records against a Python encoder written from the SAM specification (section 4.2), independent of csrc/bam_core.h; BGZF
members against zlib and the repository's own inflater.  The same corpora run through the kernels in test_bam_gpu.py."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OK, EFIELDS, ENAME, ECIGAR, ETAG, ESEQQUAL, ENOEOL, ERNAME, ENUMBER, EINT, EFLOAT, EBARRAY, ESIZE = range(13)
CONTIGS = [("chr1", 500_000_000), ("chr2", 4000), ("chr1_alt", 150), ("HLA-A*01:01", 70)]
PIECE = 0xff00


# ---------------------------------------------------------------------------------------------------------------- the record oracle

class Refused(Exception):
    pass


def reg2bin(beg, end):
    end -= 1
    for sh, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == end >> sh:
            return (base + (beg >> sh)) & 0xFFFF
    return 0


def encode_line(line: bytes, contigs) -> bytes:
    """one SAM line (no newline) -> its BAM record, block_size included; Refused(status) where the converter must refuse"""
    import re
    names = [c[0].encode() for c in contigs]
    f = line.split(b"\t")
    if len(f) < 11:
        raise Refused(EFIELDS)
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if not 1 <= len(qname) <= 254:
        raise Refused(ENAME)

    def num(b, lo, hi):
        if not re.fullmatch(rb"[-+]?[0-9]{1,18}", b) or not lo <= int(b) <= hi:
            raise Refused(ENUMBER)
        return int(b)
    flag, pos, mapq, pnext, tlen = num(flag, 0, 65535), num(pos, 0, 2**31 - 1), num(mapq, 0, 255), num(pnext, 0, 2**31 - 1), num(tlen, -2**31, 2**31 - 1)

    def ref(b):
        if b == b"*":
            return -1
        if b not in names:
            raise Refused(ERNAME)
        return names.index(b)
    rid = ref(rname)
    nid = rid if rnext == b"=" else ref(rnext)
    ops = []
    if cigar != b"*":
        if not re.fullmatch(rb"([0-9]{1,9}[MIDNSHP=X])+", cigar):
            raise Refused(ECIGAR)
        ops = [(int(a), b"MIDNSHP=X".index(o)) for a, o in re.findall(rb"([0-9]+)([MIDNSHP=X])", cigar)]
        if len(ops) > 65535 or any(a >= 1 << 28 for a, _ in ops):
            raise Refused(ECIGAR)
    l_seq = 0 if seq == b"*" else len(seq)
    if not seq or not qual or (qual != b"*" and (seq == b"*" or len(qual) != l_seq)):
        raise Refused(ESEQQUAL)
    rlen = sum(a for a, o in ops if o in (0, 2, 3, 7, 8))
    b0 = pos - 1
    bin_ = 4680 if b0 < 0 else reg2bin(b0, b0 + 1 if (flag & 4) or rlen == 0 else b0 + rlen)
    body = struct.pack("<iiBBHHHIiii", rid, b0, len(qname) + 1, mapq, bin_, len(ops), flag, l_seq, nid, pnext - 1, tlen) + qname + b"\0"
    body += b"".join(struct.pack("<I", a << 4 | o) for a, o in ops)
    nt = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
    code = [nt.get(chr(c).upper(), 15) for c in (seq if l_seq else b"")]
    body += bytes((code[i] << 4) | (code[i + 1] if i + 1 < l_seq else 0) for i in range(0, l_seq, 2))
    body += b"\xff" * l_seq if qual == b"*" else bytes(c - 33 for c in qual)
    for t in f[11:]:
        if len(t) < 5 or t[2:3] != b":" or t[4:5] != b":":
            raise Refused(ETAG)
        ty, v = t[3:4], t[5:]
        if ty == b"B":
            raise Refused(EBARRAY)
        if ty not in (b"A", b"i", b"f", b"Z", b"H"):
            raise Refused(ETAG)
        body += t[:2]
        if ty == b"A":
            if len(v) != 1:
                raise Refused(ETAG)
            body += b"A" + v
        elif ty in (b"Z", b"H"):
            body += ty + v + b"\0"
        elif ty == b"i":
            if not re.fullmatch(rb"[-+]?[0-9]{1,18}", v) or not -2**31 <= int(v) < 2**32:
                raise Refused(EINT)
            x = int(v)
            if x < 0:
                body += struct.pack("<cb", b"c", x) if x >= -128 else struct.pack("<ch", b"s", x) if x >= -32768 else struct.pack("<ci", b"i", x)
            else:
                body += struct.pack("<cB", b"C", x) if x <= 255 else struct.pack("<cH", b"S", x) if x <= 65535 else struct.pack("<cI", b"I", x)
        else:
            if not re.fullmatch(rb"[-+]?[0-9]+(\.[0-9]+)?", v) or sum(c in b"0123456789" for c in v) > 15:
                raise Refused(EFLOAT)
            body += b"f" + struct.pack("<f", float(v))                  # float(): the correctly rounded double, as strtod; 'f': rounded to float
    return struct.pack("<I", len(body)) + body


def encode_text(text: bytes, contigs):
    """(records back to back, status per line) of SAM record lines"""
    lines = text.split(b"\n")
    last_open = lines[-1] != b""
    if not last_open:
        lines.pop()
    out, st = [], []
    for i, l in enumerate(lines):
        try:
            rec = encode_line(l, contigs)
            if last_open and i == len(lines) - 1:
                raise Refused(ENOEOL)
            out.append(rec); st.append(OK)
        except Refused as e:
            st.append(e.args[0])
    return b"".join(out), np.array(st, np.uint32)


def record_corpus() -> bytes:
    base = b"r%d\t%d\t%s\t%d\t60\t%s\t%s\t%d\t%d\t%s\t%s"
    L = []
    L.append(b"plain\t0\tchr1\t100\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tNM:i:0\tMD:Z:10\tAS:i:10\tXS:i:0")
    L.append(b"stars\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*")
    L.append(b"noqual\t16\tchr2\t7\t3\t2S3M1I2M1D1M2H\t=\t300\t-150\tACGTNacgt\t*\tXA:Z:chr1,+5,9M,0;")
    L.append(b"odd\t99\tchr1\t268435457\t255\t3M2N3=1X\tchr2\t1\t2147483647\tRYKMSWB\t!~5555I")
    L.append(b"unmapped_placed\t4\tchr1\t16384\t0\t5M\t=\t16384\t0\tACGTA\tIIIII")
    L.append(b"alt\t2048\tHLA-A*01:01\t1\t0\t4M\tchr1_alt\t2\t-2147483648\tACGT\tIIII\tpa:f:0.857\tSA:Z:chr1,1,+,4M,60,0;")
    for v in (-129, -128, -1, 0, 255, 256, 65535, 65536, 2**31, -2**31, 2**31 - 1, 2**32 - 1, -32768, -32769):
        L.append(b"int%d\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXX:i:%d" % (v & 0xFFFF, v))
    L.append(b"tags\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXA:A:q\tXZ:Z:\tXH:H:1AE301\tXf:f:-12.5\tXg:f:+3\tXh:f:0.1\tXi:f:123456789.012345\tXj:f:0.000000000000001\tBC:Z:AC GT")
    L.append(b"n" * 254 + b"\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI")
    # refusals, each between records that stay right
    bad = [b"short\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA", b"n" * 255 + b"\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI", b"\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI",
           b"ops\t0\tchr1\t1\t0\t" + b"1M1I" * 32768 + b"\t*\t0\t0\t*\t*", b"cig\t0\tchr1\t1\t0\t5Q\t*\t0\t0\tA\tI", b"cig2\t0\tchr1\t1\t0\tM\t*\t0\t0\tA\tI",
           b"cig3\t0\tchr1\t1\t0\t5\t*\t0\t0\tA\tI", b"tag\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\t1:N:0:ACGT", b"tag2\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXX:q:1",
           b"tag3\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXX:A:ab", b"tag4\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tNM:i:1\t", b"sq\t0\tchr1\t1\t0\t2M\t*\t0\t0\tAC\tI",
           b"sq2\t0\tchr1\t1\t0\t*\t*\t0\t0\t*\tII", b"ref\t0\tchr9\t1\t0\t1M\t*\t0\t0\tA\tI", b"ref2\t0\tchr1\t1\t0\t1M\tchr\t0\t0\tA\tI",
           b"num\t65536\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI", b"num2\t0\tchr1\t-1\t0\t1M\t*\t0\t0\tA\tI", b"num3\t0\tchr1\t1\t256\t1M\t*\t0\t0\tA\tI",
           b"num4\t0\tchr1\t1x\t0\t1M\t*\t0\t0\tA\tI", b"int\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXX:i:4294967296", b"int2\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXX:i:-2147483649",
           b"int3\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXX:i:1.5", b"flt\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXX:f:1e-3", b"flt2\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXX:f:.5",
           b"flt3\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXX:f:1234567890.123456", b"flt4\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXX:f:inf", b"arr\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\tI\tXX:B:c,1,2", b""]
    good = L[0]
    for b in bad:
        L += [b, good]
    L.append(b"ops_ok\t0\tchr1\t1\t0\t" + b"1M1I" * 32767 + b"1M\t*\t0\t0\t*\t*")
    return b"\n".join(L) + b"\n"


def golden_sam_texts():
    """SAM record lines the repository's golden files hold (what the existing paths write), where a test can read them without a device"""
    out = []
    g = os.path.join(HERE, "golden")
    for fn in sorted(os.listdir(g)):
        if fn.endswith(".npz"):
            try:
                z = np.load(os.path.join(g, fn), allow_pickle=False)
            except Exception:
                continue
            for k in z.files:
                a = z[k]
                if a.dtype == np.uint8 and a.ndim == 1 and a.size > 200:
                    b = a.tobytes()
                    body = b"".join(l + b"\n" for l in b.split(b"\n") if l and not l.startswith(b"@"))
                    if body.count(b"\t") >= 10 * max(body.count(b"\n"), 1):
                        out.append((fn + ":" + k, b, body))
    return out


# ---------------------------------------------------------------------------------------------------------------- the member corpus

def sam_like(n_bytes: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    recs, size, i = [], 0, 0
    while size < n_bytes:
        ln = int(rng.integers(100, 152))
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), ln).tobytes()
        q = (rng.integers(0, 8, ln) * 5 + 35).astype(np.uint8).tobytes()
        r = b"r%d\t%d\tchr%d\t%d\t60\t%dM\t=\t%d\t%d\t%s\t%s\tNM:i:%d\tMD:Z:%d\tAS:i:%d\n" % (i, 99, i % 3, 1000 + 37 * i, ln, 1300 + 37 * i, 450, seq, q, i % 3, ln, ln - i % 7)
        recs.append(r); size += len(r); i += 1
    return b"".join(recs)[:n_bytes]


def far_pattern(dist: int) -> bytes:
    """200 bytes of 128 .. 255 at position 0 and again at `dist`, between and behind them random ACGT letters (which use at most 256 slots of the position table)"""
    rng = np.random.default_rng(5)
    pat = rng.integers(128, 256, 200, dtype=np.uint8).tobytes()
    fill = rng.choice(np.frombuffer(b"ACGT", np.uint8), 40000).tobytes()
    return pat + fill[:dist - 200] + pat + fill[dist:dist + 300]


def member_corpus() -> list:
    rng = np.random.default_rng(3)
    text = sam_like(210_000, 1)
    rnd = rng.integers(0, 256, 200 * 1024, dtype=np.uint8).tobytes()
    line = sam_like(4000, 2).split(b"\n")[1][:199] + b"\n"
    straddle = bytearray(rng.integers(0, 256, 4000, dtype=np.uint8).tobytes())
    straddle[50:50 + 40] = straddle[1000:1040]; straddle[1900:1900 + 300] = straddle[120:420]; straddle[-37:] = straddle[300:337]      # across step 0 / 1, steps 29 .. 34, up to the last byte
    out = [("empty", b"")]
    for n in (1, 2, 3, 64, 65):
        out += [(f"zeros {n}", b"\0" * n), (f"text {n}", text[:n])]
    out += [("zeros 0xff00", b"\0" * PIECE), ("zeros 0xff00 + 1", b"\0" * (PIECE + 1)), ("one byte repeated", b"Q" * 70001), ("all 256 values", bytes(range(256)) * 3),
            ("all 256 values once", bytes(range(256))), ("random 200 KiB", rnd), ("random 0xff00", rnd[:PIECE]), ("text 200 KiB", text[:200 * 1024]), ("text 0xff00 + 1", text[:PIECE + 1]),
            ("pattern at 32768", far_pattern(32768)), ("pattern at 32769", far_pattern(32769)), ("straddling repeats", bytes(straddle)),
            ("repeat to the last byte", text[:PIECE - 100] + text[5000:5100]), ("one line repeated", (line * 400)[:60 * 1024]), ("two values", bytes([7, 9] * 500)),
            ("ab", b"ab" * 40), ("one match", b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ!@#$%^&*()_+-=[]{}0123456789abcdefghij")]
    return out


def split_members(blob: bytes) -> list:
    out, p = [], 0
    while p < len(blob):
        assert blob[p:p + 4] == b"\x1f\x8b\x08\x04" and blob[p + 10:p + 16] == b"\x06\x00BC\x02\x00", p
        bs = struct.unpack_from("<H", blob, p + 16)[0] + 1
        out.append(blob[p:p + bs]); p += bs
    assert p == len(blob)
    return out


def check_members(blob: bytes, data: bytes, level: int, what=""):
    ms = split_members(blob)
    assert len(ms) == (len(data) + PIECE - 1) // PIECE, what
    for i, m in enumerate(ms):
        piece = data[i * PIECE:(i + 1) * PIECE]
        assert len(m) <= 65536 and len(m) <= len(piece) + 31, (what, i, len(m))
        assert zlib.decompress(m, 31) == piece, (what, i)
        crc, isize = struct.unpack("<II", m[-8:])
        assert crc == zlib.crc32(piece) and isize == len(piece) and isize > 0, (what, i)
        if level == 0:
            assert len(m) == len(piece) + 31 and m[18] == 1, (what, i)
    return ms


# ---------------------------------------------------------------------------------------------------------------- the cores under the sanitizers

def _build(name):
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    core = {"bam_core_host": ["bam_core.h"], "deflate_core_host": ["deflate_core.h", "inflate_core.h"]}[name]
    src = [os.path.join(HERE, name + ".cpp")] + [os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc", c) for c in core]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def _run(exe, fi, fo):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:verify_asan_link_order=0")
    r = subprocess.run([exe, fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    with open(fo, "rb") as f:
        return f.read()


def run_bam_core(tmp_path, text: bytes, contigs):
    from bwamem_hip.lib import _contig_table
    blob, off = _contig_table(contigs)
    lines = text.split(b"\n")
    eol = [1] * len(lines)
    if lines[-1] == b"":
        lines.pop(); eol.pop()
    else:
        eol[-1] = 0
    fi, fo = str(tmp_path / "bam_cases.bin"), str(tmp_path / "bam_results.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<II", len(contigs), len(blob)) + blob.tobytes() + off.tobytes() + struct.pack("<I", len(lines)))
        for l, e in zip(lines, eol):
            f.write(struct.pack("<II", len(l), e) + l)
    res = _run(_build("bam_core_host"), fi, fo)
    out, st, p = [], [], 0
    for _ in lines:
        s, n = struct.unpack_from("<II", res, p); p += 8
        st.append(s); out.append(res[p:p + n]); p += n
    assert p == len(res)
    return b"".join(out), np.array(st, np.uint32)


def run_deflate_core(tmp_path, data: bytes, level: int) -> bytes:
    pieces = [data[p:p + PIECE] for p in range(0, len(data), PIECE)]
    fi, fo = str(tmp_path / "dfl_cases.bin"), str(tmp_path / "dfl_results.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(pieces)))
        for pc in pieces:
            f.write(struct.pack("<II", level, len(pc)) + pc)
    res = _run(_build("deflate_core_host"), fi, fo)
    out, p = [], 0
    for _ in pieces:
        n = struct.unpack_from("<I", res, p)[0]; p += 4
        out.append(res[p:p + n]); p += n
    assert p == len(res)
    return b"".join(out)


# ---------------------------------------------------------------------------------------------------------------- records

def test_oracle_knows_the_spec_example():
    """the encoder against a record worked out by hand from the specification"""
    rec = encode_line(b"r\t16\tchr2\t7\t3\t2M\t=\t9\t-4\tAC\t!+\tNM:i:300", CONTIGS)
    want = struct.pack("<IiiBBHHHIiii", 0, 1, 6, 2, 3, 4681, 1, 16, 2, 1, 8, -4) + b"r\0" + struct.pack("<I", 2 << 4) + b"\x12" + b"\x00\x0a" + b"NMS" + struct.pack("<H", 300)
    assert rec == struct.pack("<I", len(want) - 4) + want[4:]
    assert encode_line(b"u\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*", CONTIGS)[4:16] == struct.pack("<iiBBH", -1, -1, 2, 0, 4680)


def test_records_core_under_sanitizers(tmp_path):
    text = record_corpus()
    want, want_st = encode_text(text, CONTIGS)
    assert set(want_st.tolist()) == set(range(12)) - {ENOEOL}, "the corpus holds every refusal"
    got, st = run_bam_core(tmp_path, text, CONTIGS)
    assert st.tolist() == want_st.tolist()
    assert got == want
    # the last line without its newline: refused, the records before it unchanged
    got, st = run_bam_core(tmp_path, text[:-1], CONTIGS)
    want2, want_st2 = encode_text(text[:-1], CONTIGS)
    assert st[-1] == ENOEOL and st.tolist() == want_st2.tolist() and got == want2 and want.startswith(want2)


def test_records_host_entry_point():
    from bwamem_hip.lib import BAM_STATUS, bam_status_name, sam_to_bam
    text = record_corpus()
    for t in (text, text[:-1], b"", b"\n"):
        want, want_st = encode_text(t, CONTIGS)
        got, st = sam_to_bam(t, CONTIGS, host=True)
        assert st.tolist() == want_st.tolist() and got == want
    assert len(BAM_STATUS) == 13 and "254" in bam_status_name(ENAME) and "65535" in bam_status_name(ECIGAR)


def test_records_of_golden_sam_text():
    """the SAM text stored under tests/golden (written by the existing paths): every record converts, and as the oracle says"""
    from bwamem_hip.lib import sam_to_bam
    texts = golden_sam_texts()
    for what, full, body in texts:
        contigs = [(l.split(b"\t")[1][3:].decode(), int(l.split(b"\t")[2][3:])) for l in full.split(b"\n") if l.startswith(b"@SQ")]
        if not contigs:
            contigs = sorted({(l.split(b"\t")[2].decode(), 1 << 29) for l in body.split(b"\n") if l and l.split(b"\t")[2] != b"*"} |
                             {(l.split(b"\t")[6].decode(), 1 << 29) for l in body.split(b"\n") if l and l.split(b"\t")[6] not in (b"*", b"=")})
        want, want_st = encode_text(body, contigs)
        got, st = sam_to_bam(body, contigs, host=True)
        assert not want_st.any() and not st.any(), what
        assert got == want, what


def test_bam_header():
    from bwamem_hip.lib import bam_header
    txt = "@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:c2\tLN:7\n@RG\tID:x\n"
    want = b"BAM\1" + struct.pack("<I", len(txt)) + txt.encode() + struct.pack("<I", 2) + struct.pack("<I", 5) + b"chr1\0" + struct.pack("<I", 1000) + struct.pack("<I", 3) + b"c2\0" + struct.pack("<I", 7)
    assert bam_header(txt, [("chr1", 1000), ("c2", 7)]) == want


# ---------------------------------------------------------------------------------------------------------------- members

@pytest.mark.parametrize("level", [0, 1])
def test_members_core_and_host_entry_point(tmp_path, level):
    from bwamem_hip.lib import bgzf_compress, bgzf_eof, inflate_bgzf
    assert zlib.decompress(bgzf_eof(), 31) == b"" and len(bgzf_eof()) == 28
    sizes = {}
    for name, data in member_corpus():
        blob = bgzf_compress(data, level, host=True)
        if not data:
            assert blob == b""
            continue
        ms = check_members(blob, data, level, name)
        assert run_deflate_core(tmp_path, data, level) == blob, name           # the same source under the sanitizers, in blocks of exactly their sizes
        assert bgzf_compress(data, level, host=True) == blob, name             # twice the same
        assert inflate_bgzf(blob + bgzf_eof(), host=True) == data, name       # the repository's own inflater (zlib's code-length rules)
        sizes[name] = [len(m) for m in ms]
    if level == 1:
        assert all(s <= 65536 for s in sizes["random 200 KiB"]) and sizes["random 0xff00"] == [PIECE + 31]      # stored
        assert sizes["zeros 0xff00"][0] < 600 and sizes["one byte repeated"][0] < 600
        # 200 bytes of 128 .. 255 cost some 30 bits as one match and more than 8 bits each as literals: the member that may refer to them (32 768) is
        # smaller by more than 150 bytes than the one that may not (32 769; zlib refused a distance beyond 32 768 above)
        assert sizes["pattern at 32768"][0] + 150 < sizes["pattern at 32769"][0]


def test_level_1_compresses():
    """60 KiB of one 200-byte SAM line: any LZ77 with 258-byte matches spends under 30 bits per 258 bytes there"""
    from bwamem_hip.lib import bgzf_compress
    data = dict(member_corpus())["one line repeated"]
    assert len(data) == 60 * 1024
    m = split_members(bgzf_compress(data, 1, host=True))
    assert len(m) == 1 and len(m[0]) * 4 <= len(data), len(m[0])


def test_python_keywords_refuse_bad_values():
    from bwamem_hip.lib import bgzf_compress
    with pytest.raises(ValueError):
        bgzf_compress(b"abc", 2, host=True)
