"""Duplicate marking (flag 0x400), host forms: csrc/bam_dup_core.h and csrc/bam_dup_host.cpp as plain C++ under AddressSanitizer and UBSan
(tests/bam_dup_core_host.cpp) and the library's host entry points, against a model of the rules written here from DESIGN.md 4.11 with dictionaries keyed by tuples
(no sort-and-compare: it shares no method with the code under test) and pinned itself by a table of hand-made cases whose expected bits are spelled out record by
record.  The same corpus runs on the device in test_bam_dup_gpu.py.

Every corpus member says what it must hold -- a duplicate pair, a duplicate fragment, an untouched template -- and the tests assert it from the model's answer, so
none passes vacuously.  The members of 0, 1 and 2 templates cannot hold all three (two pairs, a fragment at one's end: three templates at the least) and the
doubled golden texts hold what their reads allow (a single-end text has no pairs): their `must` sets say so."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from test_bam_core import encode_text, golden_sam_texts
from test_bam_sort import CONTIGS, BamFile, check_file, fields, make_record, split_records

HERE = os.path.dirname(os.path.abspath(__file__))
DUP = 0x400


# ---------------------------------------------------------------------------------------------------------------- records

def rec(name, rid, pos, flag, ops=((50, 0),), q=30, l_seq=None):
    """make_record with qualities: q an int (every base), a list, or None (no qualities: 0xff)"""
    if l_seq is None:
        l_seq = sum(n for n, o in ops if o in (0, 1, 4, 7, 8)) if ops else 50
    r = bytearray(make_record(rid, pos, flag, name, ops=ops, l_seq=l_seq))
    qs = bytes([0xFF] * l_seq) if q is None else bytes([q] * l_seq) if isinstance(q, int) else bytes(q)
    assert len(qs) == l_seq
    r[len(r) - l_seq:] = qs
    return bytes(r)


def pair(name, rid1, pos1, rev1, rid2, pos2, rev2, q=30, ops1=((50, 0),), ops2=((50, 0),)):
    """the two primary lines of a pair, read 1 first"""
    f1 = 0x1 | 0x40 | (0x10 if rev1 else 0) | (0x20 if rev2 else 0)
    f2 = 0x1 | 0x80 | (0x10 if rev2 else 0) | (0x20 if rev1 else 0)
    return [rec(name, rid1, pos1, f1, ops1, q), rec(name, rid2, pos2, f2, ops2, q)]


def flag_of(r: bytes) -> int:
    return struct.unpack_from("<H", r, 18)[0]


def name_of(r: bytes) -> bytes:
    return r[36:36 + r[12] - 1]


def set_dup(r: bytes) -> bytes:
    return r[:19] + bytes([r[19] | 0x04]) + r[20:]


def mask_dup(stream: bytes) -> bytes:
    return b"".join(r[:19] + bytes([r[19] & ~0x04 & 0xFF]) + r[20:] for r in split_records(stream))


# ---------------------------------------------------------------------------------------------------------------- the model

def _ops(r):
    l_name, n_ops = r[12], struct.unpack_from("<H", r, 16)[0]
    return [(v >> 4, v & 15) for v in struct.unpack_from("<%dI" % n_ops, r, 36 + l_name)]


def end_word(r):
    rid, pos, _b, fl, end = fields(r)
    ops = _ops(r)
    if not fl & 0x10:
        u = pos
        for n, o in ops:
            if o not in (4, 5):
                break
            u -= n
    else:
        u = end - 1
        for n, o in reversed(ops):
            if o not in (4, 5):
                break
            u += n
    return (rid & 0xFFFFFFFF) << 32 | ((u + (1 << 30)) & 0x7FFFFFFF) << 1 | (fl >> 4 & 1)


def score_of(r):
    l_name, n_ops = r[12], struct.unpack_from("<H", r, 16)[0]
    l_seq = struct.unpack_from("<I", r, 20)[0]
    q = r[36 + l_name + 4 * n_ops + (l_seq + 1) // 2:][:l_seq]
    return 0 if not l_seq or q[0] == 0xFF else sum(v for v in q if v >= 15)


def templates_of(recs):
    """lists of record indices; ValueError as bam_markdup refuses"""
    out = []
    for i, r in enumerate(recs):
        fl = flag_of(r)
        if not fl & 0x900 and (not fl & 1 or fl & 0x40):
            out.append([i])
        elif not out:
            raise ValueError("the first record begins no template")
        else:
            out[-1].append(i)
    return out


def model(stream: bytes):
    """(the records with 0x400 set by the rules, the counts, what the stream holds: {"pair", "frag", "clean"})"""
    recs = split_records(stream)
    tpls = templates_of(recs)
    info = []                                                  # (kind, words, score)
    for t in tpls:
        pri = [recs[i] for i in t if not flag_of(recs[i]) & 0x900]
        if flag_of(pri[0]) & 1:
            if len(pri) != 2 or {flag_of(p) & 0xC0 for p in pri} != {0x40, 0x80}:
                raise ValueError("a paired template lacks a primary line")
        elif len(pri) != 1:
            raise ValueError("an unpaired template with two primary lines")
        words = [end_word(p) for p in pri if not flag_of(p) & 4]
        info.append((len(words), tuple(sorted(words)), sum(score_of(p) for p in pri)))
    best_pair, pair_ends, best_frag = {}, set(), {}
    for o, (k, w, s) in enumerate(info):
        if k == 2:
            best_pair[w] = min(best_pair.get(w, (0, 1 << 40)), (-s, o))
            pair_ends.update(w)
        elif k == 1:
            best_frag[w] = min(best_frag.get(w, (0, 1 << 40)), (-s, o))
    dup = []
    for o, (k, w, s) in enumerate(info):
        dup.append((k == 2 and best_pair[w][1] != o) or (k == 1 and (w[0] in pair_ends or best_frag[w][1] != o)))
    out = list(recs)
    for t, d in zip(tpls, dup):
        if d:
            for i in t:
                out[i] = set_dup(out[i])
    counts = dict(pairs_examined=sum(1 for k, _w, _s in info if k == 2), fragments_examined=sum(1 for k, _w, _s in info if k == 1),
                  duplicate_pairs=sum(1 for (k, _w, _s), d in zip(info, dup) if d and k == 2), duplicate_fragments=sum(1 for (k, _w, _s), d in zip(info, dup) if d and k == 1),
                  records_flagged=sum(len(t) for t, d in zip(tpls, dup) if d), secondary_or_supplementary=sum(1 for r in recs if flag_of(r) & 0x900),
                  unmapped_records=sum(1 for r in recs if flag_of(r) & 4), templates=len(tpls))
    holds = set()
    if counts["duplicate_pairs"]:
        holds.add("pair")
    if counts["duplicate_fragments"]:
        holds.add("frag")
    if not all(dup):
        holds.add("clean")
    return b"".join(out), counts, holds


# ---------------------------------------------------------------------------------------------------------------- the table

def table():
    """[(record, expected 0x400 bit)] -- every bit written out by hand from the rules"""
    T = []

    def add(recs, bits):
        assert len(recs) == len(bits)
        T.extend(zip(recs, bits))
    # two FR pairs at one key, different scores: the better one stays although it comes second
    add(pair(b"a1", 1, 100, 0, 1, 251, 1, q=20), [1, 1])
    add(pair(b"a2", 1, 100, 0, 1, 251, 1, q=30), [0, 0])
    # the same with equal scores: the earlier one stays
    add(pair(b"b1", 1, 1000, 0, 1, 1151, 1), [0, 0])
    add(pair(b"b2", 1, 1000, 0, 1, 1151, 1), [1, 1])
    # FR against RF at the same coordinates (u = 2000 and 2300 both times, the strands exchanged): no duplicates
    add(pair(b"c1", 1, 2000, 0, 1, 2251, 1), [0, 0])
    add(pair(b"c2", 1, 1951, 1, 1, 2300, 0), [0, 0])
    # the mates swap roles: read 1 forward / read 2 reverse against read 1 reverse / read 2 forward at the same ends
    add(pair(b"d1", 1, 3000, 0, 1, 3251, 1), [0, 0])
    add(pair(b"d2", 1, 3251, 1, 1, 3000, 0), [1, 1])
    # leading hard and soft clips on a forward read: pos 4007 - 3 - 4 = 4000
    add(pair(b"e1", 1, 4000, 0, 1, 4251, 1), [0, 0])
    add(pair(b"e2", 1, 4007, 0, 1, 4251, 1, q=20, ops1=((3, 5), (4, 4), (43, 0))), [1, 1])
    # trailing clips on a reverse read: pos 5251 + 44 - 1 + 4 + 2 = 5300 = 5251 + 50 - 1
    add(pair(b"f1", 1, 5000, 0, 1, 5251, 1), [0, 0])
    add(pair(b"f2", 1, 5000, 0, 1, 5251, 1, q=20, ops2=((44, 0), (4, 4), (2, 5))), [1, 1])
    # a fragment at a pair's end (a1 / a2's forward end) is a duplicate whatever its score
    add([rec(b"g", 1, 100, 0, q=40)], [1])
    # two fragments alone at a word: the better one stays
    add([rec(b"h1", 1, 6000, 0, q=20)], [1])
    add([rec(b"h2", 1, 6000, 0, q=30)], [0])
    # a pair with one unmapped mate is a fragment; the mate is flagged with it
    add([rec(b"i1", 1, 7000, 0x1 | 0x40 | 0x8), rec(b"i1", 1, 7000, 0x1 | 0x80 | 0x4, ops=())], [0, 0])
    add([rec(b"i2", 1, 7000, 0x1 | 0x40 | 0x8, q=20), rec(b"i2", 1, 7000, 0x1 | 0x80 | 0x4, ops=(), q=20)], [1, 1])
    # both mates unmapped: never duplicates
    add([rec(b"j1", -1, -1, 0x1 | 0x40 | 0x4 | 0x8, ops=()), rec(b"j1", -1, -1, 0x1 | 0x80 | 0x4 | 0x8, ops=())], [0, 0])
    add([rec(b"j2", -1, -1, 0x1 | 0x40 | 0x4 | 0x8, ops=()), rec(b"j2", -1, -1, 0x1 | 0x80 | 0x4 | 0x8, ops=())], [0, 0])
    # a duplicate template with a supplementary and a secondary line: all four records flagged
    add(pair(b"k1", 1, 8000, 0, 1, 8251, 1), [0, 0])
    k2 = pair(b"k2", 1, 8000, 0, 1, 8251, 1, q=20)
    add([k2[0], rec(b"k2", 0, 77_000, 0x1 | 0x40 | 0x800, ops=((30, 5), (20, 0)), q=20), k2[1], rec(b"k2", 1, 30_000, 0x1 | 0x80 | 0x100 | 0x10, q=20)], [1, 1, 1, 1])
    # records without qualities score 0: the later fragment with qualities stays
    add([rec(b"l1", 1, 9000, 0, q=None)], [1])
    add([rec(b"l2", 1, 9000, 0, q=16)], [0])
    # mates on different contigs
    add(pair(b"m1", 0, 500, 0, 1, 10_000, 1), [0, 0])
    add(pair(b"m2", 0, 500, 0, 1, 10_000, 1, q=20), [1, 1])
    # u below 0: pos 2 - 5 = -3 = 0 - 3
    add([rec(b"n1", 0, 2, 0, ops=((5, 4), (45, 0)))], [0])
    add([rec(b"n2", 0, 0, 0, ops=((3, 4), (47, 0)), q=20)], [1])
    # qualities below 15 do not count: 50 x 14 scores 0, 10 x 15 scores 150
    add([rec(b"o1", 1, 11_000, 0, q=14)], [1])
    add([rec(b"o2", 1, 11_000, 0, q=[15] * 10 + [3] * 40)], [0])
    return T


def table_stream():
    return b"".join(r for r, _b in table())


# ---------------------------------------------------------------------------------------------------------------- the corpus

def synthetic(n_tpl: int, seed: int) -> bytes:
    """n_tpl templates drawn from 40 positions: FR pairs with one insert size (so a position is a key), fragments at the same positions, pairs with an unmapped
    mate, unmapped pairs, now and then a supplementary line"""
    rng = np.random.default_rng(seed)
    posn = [200 + 311 * k for k in range(40)]
    out = []
    for i in range(n_tpl):
        p = posn[int(rng.integers(0, 40))]; q = int(rng.integers(10, 41)); name = b"t%d" % i
        kind = float(rng.random())
        if i == 0 or kind < 0.55:
            rf = float(rng.random()) < 0.1
            rs = pair(name, 1, p, 1 if rf else 0, 1, p + 150, 0 if rf else 1, q=q)
            if float(rng.random()) < 0.1:
                rs.insert(1, rec(name, 0, 90_000 + i, 0x1 | 0x40 | 0x800, ops=((30, 5), (20, 0)), q=q))
            out += rs
        elif kind < 0.8:
            out.append(rec(name, 1, p + (0 if kind < 0.7 else 7), 0 if kind < 0.75 else 0x10, q=q))
        elif kind < 0.93:
            out += [rec(name, 1, p, 0x1 | 0x40 | 0x8, q=q), rec(name, 1, p, 0x1 | 0x80 | 0x4, ops=(), q=q)]
        else:
            out += [rec(name, -1, -1, 0x1 | 0x40 | 0xC, ops=(), q=q), rec(name, -1, -1, 0x1 | 0x80 | 0xC, ops=(), q=q)]
    return b"".join(out)


def one_key(n_pairs=300) -> bytes:
    """300 pairs share one key (a run of equal lanes across a workgroup boundary); the best is pair 170, then a fragment at their end and one elsewhere"""
    out = []
    for i in range(n_pairs):
        out += pair(b"p%03d" % i, 1, 700, 0, 1, 900, 1, q=35 if i == 170 else 20 + i % 10)
    out += [rec(b"fr_at_end", 1, 700, 0, q=40), rec(b"fr_alone", 1, 5, 0)]
    return b"".join(out)


def golden_doubled():
    """the golden SAM texts, each followed by itself under new names: (what, contigs, stream)"""
    out = []
    for what, full, body in golden_sam_texts():
        contigs = [(l.split(b"\t")[1][3:].decode(), int(l.split(b"\t")[2][3:])) for l in full.split(b"\n") if l.startswith(b"@SQ")]
        if not contigs:
            contigs = sorted({(l.split(b"\t")[k].decode(), (1 << 29) - 1) for l in body.split(b"\n") if l for k in (2, 6) if l.split(b"\t")[k] not in (b"*", b"=")})
        twice = body + b"".join(b"dup_" + l + b"\n" for l in body.split(b"\n") if l)
        recs, st = encode_text(twice, contigs)
        assert not st.any(), what
        out.append((what, contigs, recs))
    return out


_CORPUS = []


def corpus():
    """(what, contigs, stream, must): must = what the model's answer has to hold"""
    if not _CORPUS:
        every = {"pair", "frag", "clean"}
        _CORPUS.append(("table", CONTIGS, table_stream(), every))
        for n in (0, 1, 2, 63, 64, 65, 257, 1000):
            _CORPUS.append(("synthetic %d" % n, CONTIGS, synthetic(n, 100 + n), every if n >= 63 else set()))
        _CORPUS.append(("300 pairs at one key", CONTIGS, one_key(), every))
        for what, contigs, stream in golden_doubled():
            m = model(stream)[1]
            # a doubled text: every mapped template of the second half is a duplicate of its first; which kinds there are is the text's
            must = ({"pair"} if m["pairs_examined"] else set()) | ({"frag"} if m["fragments_examined"] else set()) | {"clean"}
            _CORPUS.append(("golden x 2: " + what, contigs, stream, must))
        assert sum(1 for c in _CORPUS if c[0].startswith("golden")) >= 3
        assert any("pair" in c[3] for c in _CORPUS if c[0].startswith("golden")) and any("frag" in c[3] for c in _CORPUS if c[0].startswith("golden"))
    return _CORPUS


_MODEL = {}


def expected(what, stream):
    """the model's answer of a corpus member, computed once and shared"""
    if what not in _MODEL:
        _MODEL[what] = model(stream)
    return _MODEL[what]


def flagged_names(stream: bytes) -> set:
    return {(name_of(r), flag_of(r)) for r in split_records(stream) if flag_of(r) & DUP}


# ---------------------------------------------------------------------------------------------------------------- tests

def test_model_on_the_table():
    recs = split_records(model(table_stream())[0])
    want = [b for _r, b in table()]
    assert [flag_of(r) >> 10 & 1 for r in recs] == want
    assert [name_of(r) for r, w in zip(recs, want) if w] == [name_of(r) for (r, _b), w in zip(table(), want) if w]


def test_corpus_is_not_vacuous():
    for what, _contigs, stream, must in corpus():
        _marked, counts, holds = expected(what, stream)
        assert must <= holds, (what, must, holds, counts)


def test_host_equals_model():
    from bwamem_hip.lib import bam_markdup
    for what, _contigs, stream, _must in corpus():
        want, counts, _h = expected(what, stream)
        got, c = bam_markdup(stream, host=True)
        assert c == counts, what
        assert got == want, what
        assert mask_dup(got) == stream, what
    got, _c = bam_markdup(table_stream(), host=True)
    assert [flag_of(r) >> 10 & 1 for r in split_records(got)] == [b for _r, b in table()]


def test_marking_is_idempotent_on_masked_input():
    from bwamem_hip.lib import bam_markdup
    s = synthetic(257, 357)
    a, ca = bam_markdup(s, host=True)
    b, cb = bam_markdup(a, host=True)                                       # (0x400 on the input is not read: set bits stay, the same ones are set)
    assert a == b and ca == cb


def bad_streams():
    p = pair(b"x", 1, 10, 0, 1, 200, 1)
    return [("a supplementary line first", rec(b"s", 1, 5, 0x800) + table_stream()),
            ("read 2 first", p[1] + p[0]),
            ("no 0x80 primary line", p[0] + rec(b"y", 1, 5, 0)),
            ("no 0x80 primary line at the end", table_stream() + p[0]),
            ("two 0x40 lines", p[0] + p[0]),
            ("a cut record", table_stream()[:-1]),
            ("a cut record", table_stream()[:-30]),
            ("qualities outside the record", struct.pack("<I", len(make_record(1, 5, 0, b"q")) - 14) + make_record(1, 5, 0, b"q")[4:-10])]


def test_refusals():
    from bwamem_hip.lib import bam_markdup
    for what, s in bad_streams():
        with pytest.raises(ValueError):
            bam_markdup(s, host=True)
        if what in ("a supplementary line first", "read 2 first", "no 0x80 primary line"):
            with pytest.raises(ValueError):
                model(s)
    with pytest.raises(ValueError, match="first record begins no template"):
        bam_markdup(bad_streams()[0][1], host=True)
    with pytest.raises(ValueError, match="lacks one of its two primary lines"):
        bam_markdup(bad_streams()[2][1], host=True)


@pytest.mark.parametrize("window", [0, 1, 7, 100])
def test_sorted_file_host(window):
    from bwamem_hip.lib import bam_sorted_file
    hdr = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:x\tLN:1\n"
    for what, contigs, stream, _must in corpus():
        want, counts, _h = expected(what, stream)
        bam, bai, c = bam_sorted_file(hdr, contigs, stream, 1, window, host=True, markdup=True)
        assert c == counts, what
        f = check_file(bam, bai, hdr, contigs, want, (what, window), n_regions=10)           # the sorted file of the records as the model flags them
        plain = BamFile(bam_sorted_file(hdr, contigs, stream, 1, window, host=True)[0])
        assert mask_dup(f.stream) == plain.stream, what
        assert flagged_names(f.stream) == flagged_names(want), what


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_dup_core_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_dup_core_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_dup_core.h", "bam_dup.h", "bam_dup_host.cpp", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def run_core(tmp_path, streams):
    fi, fo = str(tmp_path / "dup_case.bin"), str(tmp_path / "dup_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(streams)) + b"".join(struct.pack("<Q", len(s)) + s for s in streams))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:verify_asan_link_order=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    with open(fo, "rb") as f:
        res = f.read()
    out, p = [], 0
    for _s in streams:
        rc = struct.unpack_from("<i", res, p)[0]; p += 4
        if rc != 0:
            out.append((rc, None, None))
            continue
        n = struct.unpack_from("<I", res, p)[0]; p += 4
        flags = struct.unpack_from("<%dH" % n, res, p); p += 2 * n
        out.append((0, flags, struct.unpack_from("<8Q", res, p))); p += 64
    assert p == len(res)
    return out


def test_core_under_sanitizers(tmp_path):
    from bwamem_hip.lib import MARKDUP_COUNTS
    members = corpus()
    res = run_core(tmp_path, [c[2] for c in members])
    for (what, _contigs, stream, _must), (rc, flags, counts) in zip(members, res):
        want, wc, _h = expected(what, stream)
        assert rc == 0 and list(flags) == [flag_of(r) for r in split_records(want)], what
        assert dict(zip(MARKDUP_COUNTS, counts)) == wc, what
    assert [rc for rc, _f, _c in run_core(tmp_path, [s for _w, s in bad_streams()])] == [-2] * len(bad_streams())
    # 2000 damaged streams: bytes of the table and of a synthetic stream overwritten, cut or repeated -- refused or marked, never out of bounds
    rng = np.random.default_rng(3)
    base = [table_stream(), synthetic(65, 9)]
    damaged = []
    for k in range(2000):
        s = bytearray(base[k & 1])
        for _ in range(int(rng.integers(1, 6))):
            i = int(rng.integers(0, len(s)))
            s[i] = int(rng.integers(0, 256))
        if k % 5 == 0:
            s = s[:int(rng.integers(0, len(s)))]
        damaged.append(bytes(s))
    res = run_core(tmp_path, damaged)
    assert len(res) == 2000 and all(rc in (0, -2) for rc, _f, _c in res) and any(rc == 0 for rc, _f, _c in res) and any(rc == -2 for rc, _f, _c in res)


# ---------------------------------------------------------------------------------------------------------------- the Python keywords

def test_python_keywords(monkeypatch):
    from bwamem_hip.aligner import Aligner, markdup_metrics_text
    al = Aligner.__new__(Aligner)                                         # the keyword checks come before anything touches an index or a device
    al.profile = False
    for call in (lambda: al.align_file("r.fa", io.BytesIO(), fmt="bam", markdup=True),                  # markdup needs sort
                 lambda: al.align_file("r.fa", io.BytesIO(), markdup=True),
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", markdup=True),
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, markdup_metrics=io.StringIO()),      # metrics need markdup
                 lambda: al.align_batch(["r"], ["ACGT"], markdup=True),
                 lambda: al.align_batch(["r"], ["ACGT"], fmt="bam", sort=True, markdup=True)):
        with pytest.raises(ValueError):
            call()
    assert getattr(al, "_out_fmt", ("sam", 1)) == ("sam", 1) and not getattr(al, "_markdup", False)
    al.profile = True                                                     # a refused sorted run leaves the aligner as it was, the marking included
    with pytest.raises(NotImplementedError):
        al.align_file("r.fa", io.BytesIO(), fmt="bam", sort=True, markdup=True)
    assert getattr(al, "_out_fmt", ("sam", 1)) == ("sam", 1) and not getattr(al, "_markdup", False)
    counts = dict(pairs_examined=10, fragments_examined=4, duplicate_pairs=3, duplicate_fragments=1, records_flagged=8, secondary_or_supplementary=2, unmapped_records=5, templates=20)
    lines = markdup_metrics_text(counts, "@RG\tID:x\tLB:lib7\tSM:s").split("\n")
    assert lines[0].startswith("## METRICS CLASS") and lines[3] == ""
    row = dict(zip(lines[1].split("\t"), lines[2].split("\t")))
    assert lines[1].split("\t") == ["LIBRARY", "UNPAIRED_READS_EXAMINED", "READ_PAIRS_EXAMINED", "SECONDARY_OR_SUPPLEMENTARY_RDS", "UNMAPPED_READS", "UNPAIRED_READ_DUPLICATES",
                                    "READ_PAIR_DUPLICATES", "PERCENT_DUPLICATION"]
    assert row["LIBRARY"] == "lib7" and (int(row["UNPAIRED_READS_EXAMINED"]), int(row["READ_PAIRS_EXAMINED"]), int(row["UNPAIRED_READ_DUPLICATES"]), int(row["READ_PAIR_DUPLICATES"])) == (4, 10, 1, 3)
    assert abs(float(row["PERCENT_DUPLICATION"]) - 7 / 24) < 1e-6 and (int(row["SECONDARY_OR_SUPPLEMENTARY_RDS"]), int(row["UNMAPPED_READS"])) == (2, 5)
    empty = markdup_metrics_text(dict.fromkeys(counts, 0)).split("\n")[2].split("\t")
    assert empty[0] == "Unknown Library" and empty[-1] == "0"


def test_mem_command_refuses_markdup_without_sort(capsys):
    from bwamem_hip import mem
    assert mem.main(["--markdup", "prefix", "reads.fa"]) == 2
    assert mem.main(["--sort", "--markdup-metrics", "m.txt", "prefix", "reads.fa"]) == 2
    assert "--markdup needs --sort" in capsys.readouterr().err
