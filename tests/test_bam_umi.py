"""Barcode-aware duplicate keys (UMIs), host forms: bam_markdup(host=True, barcode_tag=... / barcode_name=True), bam_dup_barcodes, barcode_word,
bam_sorted_file and the refusals -- against a model written here from the rules.  The model groups the templates by their exact barcode strings (and, with read
groups, by library) and runs test_bam_dup.model on every group on its own: it never computes a hash, so it does not depend on the barcode word; the optical counts
come from test_bam_optical.optical_model on the same groups.  Every hand-made case also spells out the flags it must give.  tests/bam_dup_umi_host.cpp runs the
same host forms as plain C++ under AddressSanitizer and UBSan.  The corpus runs on the device in test_bam_umi_gpu.py.

Every call that passes barcode_tag= or barcode_name= raises TypeError on a tree without the feature."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from test_bam_dup import CONTIGS, flag_of, mask_dup, model, name_of, pair, rec, templates_of
from test_bam_optical import nm, optical_model
from test_bam_sort import BamFile, check_file, split_records

HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = [(b"laneA", "lib1"), (b"laneB", "lib1"), (b"other", "lib2")]
COUNT_KEYS = ("pairs_examined", "fragments_examined", "duplicate_pairs", "duplicate_fragments", "records_flagged", "secondary_or_supplementary", "unmapped_records", "templates")
OPT_KEYS = ("optical_duplicate_pairs", "located_pairs", "optical_sets_skipped")
WIDTH = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


# ---------------------------------------------------------------------------------------------------------------- records

def with_aux(r: bytes, aux: bytes) -> bytes:
    """the record with raw tag bytes behind what it holds"""
    body = r[4:] + aux
    return struct.pack("<I", len(body)) + body


def z(tag: bytes, value: bytes) -> bytes:
    return tag + b"Z" + value + b"\0"


def renamed(r: bytes, name: bytes) -> bytes:
    """the record under another read name"""
    body = r[4:12] + bytes([len(name) + 1]) + r[13:36] + name + b"\0" + r[36 + r[12]:]
    return struct.pack("<I", len(body)) + body


def upair(name, pos1, pos2, umi=None, q=30, rg=None, tag=b"RX", swap=False):
    """a pair with ends at pos1 (forward) and pos2 (reverse) whose two records carry RG:Z (rg) and the barcode tag (umi: bytes; None: no tag)"""
    p = pair(name, 1, pos2, 1, 1, pos1, 0, q=q) if swap else pair(name, 1, pos1, 0, 1, pos2, 1, q=q)
    aux = (z(b"RG", rg) if rg is not None else b"") + (z(tag, umi) if umi is not None else b"")
    return [with_aux(r, aux) for r in p]


def ufrag(name, pos, umi=None, q=30, rg=None, tag=b"RX", rev=False):
    aux = (z(b"RG", rg) if rg is not None else b"") + (z(tag, umi) if umi is not None else b"")
    return [with_aux(rec(name, 1, pos, 0x10 if rev else 0, q=q), aux)]


def join(tpls) -> bytes:
    return b"".join(r for t in tpls for r in t)


# ---------------------------------------------------------------------------------------------------------------- the model

def aux_fields(r: bytes):
    """[(tag, type, value bytes)] by a walk over the record's tags"""
    l_name, n_ops, l_seq = r[12], struct.unpack_from("<H", r, 16)[0], struct.unpack_from("<I", r, 20)[0]
    p = 36 + l_name + 4 * n_ops + (l_seq + 1) // 2 + l_seq
    out = []
    while p < len(r):
        t, ty = r[p:p + 2], chr(r[p + 2]); p += 3
        if ty in "ZH":
            e = r.index(b"\0", p)
            out.append((t, ty, r[p:e])); p = e + 1
        elif ty == "B":
            n = 5 + WIDTH[chr(r[p])] * struct.unpack_from("<I", r, p + 1)[0]
            out.append((t, ty, r[p:p + n])); p += n
        else:
            out.append((t, ty, r[p:p + WIDTH[ty]])); p += WIDTH[ty]
    return out


def barcode_of(r: bytes, tag=None, name=False):
    """the barcode string of a template's first record by the rules; None: no barcode"""
    if name:
        n = name_of(r)
        v = n.rsplit(b":", 1)[1] if b":" in n else b""
    else:
        v = next((val for t, ty, val in aux_fields(r) if t == (tag if isinstance(tag, bytes) else tag.encode()) and ty == "Z"), b"")
    return v or None


def rg_id(r: bytes):
    return next((val for t, ty, val in aux_fields(r) if t == b"RG" and ty == "Z"), None)


def umi_model(stream: bytes, tag=None, name=False, read_groups=None, optical_distance=None, optical_max_set=None):
    """(the records with 0x400 set, the counts as bam_markdup returns them, the barcode strings per template): test_bam_dup.model on the templates of every (library,
    barcode string) on their own; the optical counts from optical_model on the same groups, in name mode on the records under the names without their last field"""
    recs = split_records(stream)
    tpls = templates_of(recs)
    lib_of = dict(read_groups) if read_groups is not None else {}
    libs = list(dict.fromkeys(lb for _id, lb in read_groups)) if read_groups is not None else [None]
    members, strings = {}, []
    for idx in tpls:
        first = recs[idx[0]]
        bc = barcode_of(first, tag, name)
        strings.append(bc)
        members.setdefault((lib_of[rg_id(first)] if read_groups is not None else None, bc), []).append(idx)
    out = list(recs)
    per = {lb: dict.fromkeys(COUNT_KEYS, 0) for lb in libs}
    if optical_distance is not None:
        for lb in libs:
            per[lb].update(dict.fromkeys(OPT_KEYS, 0))
    for (lb, _bc), group in members.items():
        flat = [i for idx in group for i in idx]
        marked, counts, _h = model(b"".join(recs[i] for i in flat))
        for i, r in zip(flat, split_records(marked)):
            out[i] = r
        for k in COUNT_KEYS:
            per[lb][k] += counts[k]
        if optical_distance is not None:
            sub = [recs[i] for i in flat]
            if name:
                sub = [renamed(r, name_of(r).rsplit(b":", 1)[0]) if b":" in name_of(r) else r for r in sub]
            total, _per, _st = optical_model(b"".join(sub), optical_distance, optical_max_set or 300_000, read_groups)
            for k in OPT_KEYS:
                per[lb][k] += total[k]
    counts = {k: sum(per[lb][k] for lb in libs) for k in per[libs[0]]}
    counts["templates_without_barcode"] = sum(1 for s in strings if s is None)
    if read_groups is not None:
        counts["libraries"] = per
    return b"".join(out), counts, strings


def flags(stream: bytes):
    return [flag_of(r) >> 10 & 1 for r in split_records(stream)]


def fnv1a(v: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in v:
        h = ((h ^ b) * 0x100000001b3) & (1 << 64) - 1
    return 0 if not v else h or 1


# ---------------------------------------------------------------------------------------------------------------- hand-made cases

LONG_A, LONG_B = b"ACGT" * 75, b"ACGT" * 74 + b"ACGA"                     # 300 bytes, different in the last one


def cases():
    """[(what, stream, keywords, the 0x400 bit of every record, templates without a barcode)] -- every bit written out by hand from the rules"""
    out = []

    def add(what, tpls, bits, none=0, **kw):
        kw = kw or dict(barcode_tag="RX")
        s = join(tpls)
        assert len(split_records(s)) == len(bits), what
        out.append((what, s, kw, bits, none))
    # the pair table
    add("two pairs, one key, different barcodes", [upair(b"a1", 100, 300, b"AAAA", q=20), upair(b"a2", 100, 300, b"CCCC")], [0, 0, 0, 0])
    add("two pairs, one key, one barcode", [upair(b"a1", 100, 300, b"AAAA", q=20), upair(b"a2", 100, 300, b"AAAA")], [1, 1, 0, 0])
    add("three pairs: A, A, B", [upair(b"a1", 100, 300, b"A"), upair(b"a2", 100, 300, b"A"), upair(b"a3", 100, 300, b"B", q=10)], [0, 0, 1, 1, 0, 0])
    add("the last byte differs", [upair(b"a1", 100, 300, b"ACGTACGA"), upair(b"a2", 100, 300, b"ACGTACGC")], [0, 0, 0, 0])
    add("only the case differs", [upair(b"a1", 100, 300, b"acgt"), upair(b"a2", 100, 300, b"ACGT")], [0, 0, 0, 0])
    add("one a prefix of the other", [upair(b"a1", 100, 300, b"ACGT"), upair(b"a2", 100, 300, b"ACGTA"), upair(b"a3", 100, 300, b"ACGT")], [0, 0, 0, 0, 1, 1])
    add("a dual barcode is one value", [upair(b"a1", 100, 300, b"ACGT-TTGA"), upair(b"a2", 100, 300, b"ACGT-TTGC"), upair(b"a3", 100, 300, b"ACGT-TTGA", q=40)], [1, 1, 0, 0, 0, 0])
    add("values of 1 byte", [upair(b"a1", 100, 300, b"A"), upair(b"a2", 100, 300, b"C"), upair(b"a3", 100, 300, b"A")], [0, 0, 0, 0, 1, 1])
    add("values of 300 bytes", [upair(b"a1", 100, 300, LONG_A), upair(b"a2", 100, 300, LONG_B), upair(b"a3", 100, 300, LONG_A), upair(b"a4", 100, 300, LONG_B, q=40)],
        [0, 0, 1, 1, 1, 1, 0, 0])
    add("equal barcodes at different keys", [upair(b"a1", 100, 300, b"AAAA"), upair(b"a2", 100, 301, b"AAAA")], [0, 0, 0, 0])
    # the fragment table
    add("a fragment at a pair's end, one barcode", [upair(b"p", 100, 300, b"AA"), ufrag(b"f", 100, b"AA", q=40)], [0, 0, 1])
    add("a fragment at a pair's end, another barcode", [upair(b"p", 100, 300, b"AA"), ufrag(b"f", 100, b"CC")], [0, 0, 0])
    add("a fragment at a pair's reverse end", [upair(b"p", 100, 300, b"AA"), ufrag(b"f", 300, b"AA", rev=True), ufrag(b"g", 300, b"CC", rev=True)], [0, 0, 1, 0])
    add("two fragments, one end, different barcodes", [ufrag(b"f1", 100, b"AA", q=20), ufrag(b"f2", 100, b"CC")], [0, 0])
    add("two fragments, one end, one barcode", [ufrag(b"f1", 100, b"AA", q=20), ufrag(b"f2", 100, b"AA")], [1, 0])
    add("another barcode's pair does not hide the best fragment", [upair(b"p", 100, 300, b"GG"), ufrag(b"f1", 100, b"AA"), ufrag(b"f2", 100, b"AA", q=20)], [0, 0, 0, 1])
    # no barcode
    add("no tag and an empty tag are one kind, apart from a barcoded template",
        [upair(b"a1", 100, 300, None, q=40), upair(b"a2", 100, 300, b""), upair(b"a3", 100, 300, b"AC"), ufrag(b"f", 100, None), ufrag(b"g", 100, b"AC"), ufrag(b"h", 100, b"TT")],
        [0, 0, 1, 1, 0, 0, 1, 1, 0], none=3)
    # the tag walk
    arr = b"XBBS" + struct.pack("<I", 3) + struct.pack("<3H", 1, 2, 3)
    scal = b"XaAq" + b"Xbc\x01" + b"XcC\x02" + b"Xds\x03\x00" + b"XeS\x04\x00" + b"Xfi" + struct.pack("<i", -5) + b"XgI" + struct.pack("<I", 6) + b"Xhf" + struct.pack("<f", 1.5) + b"XiHABCD\0"
    two = [pair(b"a%d" % k, 1, 100, 0, 1, 251, 1) for k in range(3)]
    add("behind a B array", [[with_aux(r, arr + z(b"RX", b"AC")) for r in two[0]], [with_aux(r, arr + z(b"RX", b"AC")) for r in two[1]], [with_aux(r, arr + z(b"RX", b"AG")) for r in two[2]]],
        [0, 0, 1, 1, 0, 0])
    add("behind tags of every scalar width", [[with_aux(r, scal + z(b"RX", b"AC")) for r in two[0]], [with_aux(r, scal + z(b"RX", b"AC")) for r in two[1]], [with_aux(r, scal + z(b"RX", b"AG")) for r in two[2]]],
        [0, 0, 1, 1, 0, 0])
    add("another tag's name", [upair(b"a1", 100, 300, b"AC", tag=b"BC"), upair(b"a2", 100, 300, b"AC", tag=b"BC"), upair(b"a3", 100, 300, b"AG", tag=b"BC")], [0, 0, 1, 1, 0, 0],
        barcode_tag="BC")
    add("the barcode of the first record counts", [[with_aux(two[0][0], z(b"RX", b"AC")), with_aux(two[0][1], z(b"RX", b"GG"))], [with_aux(two[1][0], z(b"RX", b"AC")), two[1][1]]], [0, 0, 1, 1])
    add("RG:Z and a barcode: one barcode in two libraries",
        [upair(b"a1", 100, 300, b"AC", rg=b"laneA"), upair(b"a2", 100, 300, b"AC", rg=b"other"), upair(b"a3", 100, 300, b"AC", rg=b"laneB"), upair(b"a4", 100, 300, b"AG", rg=b"laneA")],
        [0, 0, 0, 0, 1, 1, 0, 0], barcode_tag="RX", read_groups=GROUPS)
    # name mode
    for nf, pre in ((5, b"M:1:"), (7, b"M:7:FC:1:"), (8, b"M:7:FC:1:11:")):
        add("the last of %d fields" % nf, [pair(pre + b"5:6:ACGT", 1, 100, 0, 1, 251, 1), pair(pre + b"5:6:ACGA", 1, 100, 0, 1, 251, 1), pair(pre + b"9:9:ACGT", 1, 100, 0, 1, 251, 1)],
            [0, 0, 0, 0, 1, 1], barcode_name=True)
    add("names without ':' and names that end in ':'", [pair(b"plain1", 1, 100, 0, 1, 251, 1), pair(b"other:", 1, 100, 0, 1, 251, 1), pair(b"x:AC", 1, 100, 0, 1, 251, 1), pair(b"y:AC", 1, 100, 0, 1, 251, 1)],
        [0, 0, 1, 1, 0, 0, 1, 1], none=2, barcode_name=True)
    add("name mode reads no tag", [upair(b"n:AC", 100, 300, b"TT"), upair(b"m:AC", 100, 300, b"GG")], [0, 0, 1, 1], barcode_name=True)
    add("no templates", [], [])
    return out


# ---------------------------------------------------------------------------------------------------------------- the synthetic stream

UMIS = (b"ACGTAC", b"ACGTAA", b"TTGACA-GGA", b"acgtac")


def reads(n=2000, seed=5, n_pos=30):
    """n logical templates on n_pos positions: pairs (both roles), fragments and pairs with an unmapped mate, one of four barcodes or now and then none, one of three
    read groups, a location in a small space (a third of the pairs are copies of an earlier pair of their position a few pixels away)"""
    rng = np.random.default_rng(seed)
    out, seen = [], {}
    for k in range(n):
        pos = int(rng.integers(0, n_pos))
        u = int(rng.integers(0, 12))
        umi = UMIS[u % 4] if u < 11 else None
        kind = float(rng.random())
        rg = GROUPS[int(rng.integers(0, 3))][0]
        swap = bool(rng.integers(0, 4) == 0)
        tile, x, y = int(rng.integers(1, 3)), int(rng.integers(0, 300)), int(rng.integers(0, 300))
        if kind < 0.6 and seen.get(pos) and rng.integers(0, 3) == 0:
            umi, rg, swap, tile, x, y = seen[pos][int(rng.integers(0, len(seen[pos])))]
            x, y = max(0, x + int(rng.integers(-15, 16))), max(0, y + int(rng.integers(-15, 16)))
        if kind < 0.6:
            seen.setdefault(pos, []).append((umi, rg, swap, tile, x, y))
        out.append(dict(kind="pair" if kind < 0.6 else "frag" if kind < 0.85 else "half", pos=1000 + 37 * pos, q=int(rng.integers(15, 40)), umi=umi, rg=rg, swap=swap,
                        loc=(tile, x, y), k=k, seven=bool(k & 1)))
    return out


def render(rs, mode: str, groups: bool) -> bytes:
    """the templates as records: mode "tag" -- the barcode as RX:Z, names of 5 or 7 fields; "name" -- the barcode as one more field of the name"""
    out = []
    for d in rs:
        name = nm(*d["loc"], seven=d["seven"], k=d["k"])
        aux = z(b"RG", d["rg"]) if groups else b""
        if mode == "tag":
            aux += z(b"RX", d["umi"]) if d["umi"] is not None else b""
        elif d["umi"] is not None:
            name += b":" + d["umi"]
        else:
            name = b"nofield%d" % d["k"]                                # (a name without ':' -- in tag mode the same template has a location: only the barcode runs compare)
        if d["kind"] == "pair":
            p = pair(name, 1, d["pos"] + 200, 1, 1, d["pos"], 0, q=d["q"]) if d["swap"] else pair(name, 1, d["pos"], 0, 1, d["pos"] + 200, 1, q=d["q"])
        elif d["kind"] == "frag":
            p = [rec(name, 1, d["pos"], 0, q=d["q"])]
        else:
            p = [rec(name, 1, d["pos"], 0x1 | 0x40 | 0x8, q=d["q"]), rec(name, 1, d["pos"], 0x1 | 0x80 | 0x4, ops=(), q=d["q"])]
        out.append([with_aux(r, aux) for r in p])
    return join(out)


_STREAMS, _MODELS = {}, {}


def corpus_stream(mode: str, groups: bool) -> bytes:
    if (mode, groups) not in _STREAMS:
        _STREAMS[(mode, groups)] = render(reads(), mode, groups)
    return _STREAMS[(mode, groups)]


def corpus_kw(mode: str, groups: bool, optical: bool) -> dict:
    kw = dict(barcode_tag="RX") if mode == "tag" else dict(barcode_name=True)
    if groups:
        kw["read_groups"] = GROUPS
    if optical:
        kw.update(optical_distance=25, optical_max_set=8)
    return kw


def corpus_expected(mode: str, groups: bool, optical: bool):
    """the model's answer on a corpus member, computed once and shared"""
    key = (mode, groups, optical)
    if key not in _MODELS:
        kw = corpus_kw(mode, groups, optical)
        _MODELS[key] = umi_model(corpus_stream(mode, groups), tag=kw.get("barcode_tag"), name=kw.get("barcode_name", False), read_groups=kw.get("read_groups"),
                                 optical_distance=kw.get("optical_distance"), optical_max_set=kw.get("optical_max_set"))
    return _MODELS[key]


CORPUS = [(m, g, o) for m in ("tag", "name") for g in (False, True) for o in (False, True)]


def sorted_file_stream() -> bytes:
    """the first 250 templates of the tagged corpus with read groups"""
    return render(reads()[:250], "tag", True)


# ---------------------------------------------------------------------------------------------------------------- the tests

def test_barcode_word():
    from bwamem_hip.lib import barcode_word
    assert barcode_word(b"") == 0
    assert barcode_word(b"a") == 0xaf63dc4c8601ec8c and barcode_word("foobar") == 0x85944171f73967e8      # FNV-1a's published vectors
    rng = np.random.default_rng(1)
    for n in (1, 2, 7, 8, 9, 63, 300, 5000):
        v = bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist())
        assert barcode_word(v) == fnv1a(v), n
    assert barcode_word(b"ACGT") != barcode_word(b"acgt") and barcode_word(b"ACGT-TTGA") != barcode_word(b"ACGT")


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_hand_made_cases_host(case):
    from bwamem_hip.lib import bam_markdup
    what, stream, kw, bits, none = case
    got, c = bam_markdup(stream, host=True, **kw)
    assert flags(got) == bits, what
    assert c["templates_without_barcode"] == none, what
    want, counts, _s = umi_model(stream, tag=kw.get("barcode_tag"), name=kw.get("barcode_name", False), read_groups=kw.get("read_groups"))
    assert flags(want) == bits, what                                  # (the model is pinned by the same hand-written bits)
    assert got == want and c == counts, what


def test_one_barcode_in_two_libraries_counts():
    from bwamem_hip.lib import bam_markdup
    case = next(c for c in cases() if c[0].startswith("RG:Z and a barcode"))
    _got, c = bam_markdup(case[1], host=True, **case[2])
    assert c["libraries"]["lib1"]["duplicate_pairs"] == 1 and c["libraries"]["lib2"]["duplicate_pairs"] == 0 and c["libraries"]["lib1"]["pairs_examined"] == 3


def test_optical_in_name_mode_equals_tag_mode():
    """8-field names: located by their 7 leading fields, their counts those of the same reads with the field cut off and the barcode given as a tag"""
    from bwamem_hip.lib import bam_markdup
    rs = [dict(d, seven=True) for d in reads() if d["umi"] is not None]
    tag7_s, name_s = render(rs, "tag", True), render(rs, "name", True)
    assert all(name_of(r).count(b":") == 7 for r in split_records(name_s))
    kw = dict(read_groups=GROUPS, optical_distance=25, optical_max_set=8)
    a, ca = bam_markdup(tag7_s, host=True, barcode_tag="RX", **kw)
    b, cb = bam_markdup(name_s, host=True, barcode_name=True, **kw)
    assert ca == cb and ca["optical_duplicate_pairs"] > 0 and ca["located_pairs"] == ca["pairs_examined"]
    assert flags(a) == flags(b)
    _c, cc = bam_markdup(name_s, host=True, **kw)                        # without the option an 8-field name has no location
    assert cc["located_pairs"] == 0


@pytest.mark.parametrize("mode,groups,optical", CORPUS)
def test_corpus_host_equals_model(mode, groups, optical):
    from bwamem_hip.lib import bam_markdup
    stream, kw = corpus_stream(mode, groups), corpus_kw(mode, groups, optical)
    want, counts, _strings = corpus_expected(mode, groups, optical)
    got, c = bam_markdup(stream, host=True, **kw)
    assert c == counts
    assert got == want
    plain_kw = {k: v for k, v in kw.items() if not k.startswith("barcode")}
    plain, pc = bam_markdup(stream, host=True, **plain_kw)
    n_with, n_without = c["duplicate_pairs"] + c["duplicate_fragments"], pc["duplicate_pairs"] + pc["duplicate_fragments"]
    assert 0 < n_with < n_without, (n_with, n_without)                # barcodes rescue templates, and leave duplicates
    assert 0 < c["templates_without_barcode"] < c["templates"]
    if optical:
        assert c["optical_duplicate_pairs"] > 0 and c["optical_sets_skipped"] > 0 and 0 < c["located_pairs"] <= c["pairs_examined"]


def test_without_the_option_nothing_changes():
    from bwamem_hip.lib import bam_markdup
    for groups in (False, True):
        s = corpus_stream("tag", groups)
        kw = dict(read_groups=GROUPS) if groups else {}
        assert bam_markdup(s, host=True, **kw) == bam_markdup(s, host=True, barcode_tag=None, **kw) == bam_markdup(s, host=True, barcode_tag=None, barcode_name=False, **kw)
        assert "templates_without_barcode" not in bam_markdup(s, host=True, **kw)[1]


@pytest.mark.parametrize("mode", ("tag", "name"))
def test_barcode_words_host(mode):
    from bwamem_hip.lib import bam_dup_barcodes, barcode_word
    s = corpus_stream(mode, True)
    _m, _c, strings = corpus_expected(mode, True, False)
    got = bam_dup_barcodes(s, host=True, **(dict(tag="RX") if mode == "tag" else dict(name=True)))
    assert got.dtype == np.uint64 and got.tolist() == [barcode_word(v or b"") for v in strings]
    assert len(set(got.tolist())) == 5                                 # four barcodes and none


@pytest.mark.parametrize("window", (0, 1, 7, 100))
def test_sorted_file_host(window):
    from bwamem_hip.lib import bam_sorted_file
    hdr = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:x\tLN:1\n"
    s = sorted_file_stream()
    want, counts, _strings = umi_model(s, tag="RX", read_groups=GROUPS)
    bam, bai, c = bam_sorted_file(hdr, CONTIGS, s, 1, window, host=True, markdup=True, read_groups=GROUPS, barcode_tag="RX")
    assert c == counts
    f = check_file(bam, bai, hdr, CONTIGS, want, ("barcodes", window), n_regions=10)      # the sorted file of the records as the model flags them
    plain = bam_sorted_file(hdr, CONTIGS, s, 1, window, host=True, markdup=True, read_groups=GROUPS)
    assert mask_dup(f.stream) == mask_dup(BamFile(plain[0]).stream)
    assert plain[2]["duplicate_pairs"] > c["duplicate_pairs"] > 0 and "templates_without_barcode" not in plain[2]
    bam2, csi, c2 = bam_sorted_file(hdr, CONTIGS, s, 1, window, host=True, markdup=True, read_groups=GROUPS, barcode_tag="RX", index_format="csi")
    assert bam2 == bam and c2 == c and csi != bai


def test_refusals():
    from bwamem_hip.lib import _err, bam_dup_barcodes, bam_markdup, bam_sorted_file, load_library
    s = join([upair(b"a1", 100, 300, b"AC"), upair(b"a2", 100, 300, b"AC")])
    for bad in ("R", "RXX", "1X", "X-", "X_", "", "RG", "NM", "MD", "AS", "XS", "SA", "XA", "pa", b"\xc4X", 5):
        with pytest.raises(ValueError):
            bam_markdup(s, host=True, barcode_tag=bad)
        with pytest.raises(ValueError):
            bam_dup_barcodes(s, host=True, tag=bad)
    with pytest.raises(ValueError, match="one"):
        bam_markdup(s, host=True, barcode_tag="RX", barcode_name=True)
    with pytest.raises(ValueError, match="markdup"):
        bam_sorted_file("@HD\tVN:1.6\n", CONTIGS, s, host=True, barcode_tag="RX")
    with pytest.raises(ValueError, match="markdup"):
        bam_sorted_file("@HD\tVN:1.6\n", CONTIGS, s, host=True, barcode_name=True)
    with pytest.raises(ValueError):
        bam_dup_barcodes(s, host=True)
    # the library's own check, behind Python's
    L = load_library()
    from bwamem_hip.lib import MarkdupOpt, MarkdupCounts, _markdup_api
    _markdup_api(L)
    out, res = C.c_void_p(), MarkdupCounts()

    def call(mode, tag, r=res):
        o = MarkdupOpt()
        L.bmh_markdup_opt_default(C.byref(o))
        o.barcode_mode, o.barcode_tag = mode, tag or b""
        return L.bmh_bam_markdup_host(s, len(s), C.byref(o), C.byref(out), C.byref(r) if r is not None else None)
    for mode, tag in ((1, b"RG"), (1, b"pa"), (1, b"1X"), (1, b"X-"), (1, b"X"), (1, None), (3, b"RX"), (-1, b"RX")):
        assert call(mode, tag) == -2, (mode, tag)
        assert out.value is None and ("barcode" in _err(L))
    assert call(1, b"RX", None) == -2 and out.value is None             # (a call without its counts record)
    assert call(1, b"RX") == 0 and res.counts[2] == 1
    L.bmh_free.argtypes = [C.c_void_p]; L.bmh_free(out)
    # records: a tag of another type, tags that cannot be walked -- by the index of the template's first record
    good = upair(b"g", 100, 300, b"AC")
    p = pair(b"b", 1, 100, 0, 1, 251, 1)
    for what, aux, word in (("an integer", b"RXi" + struct.pack("<i", 7), "type"), ("hex", b"RXHAB\0", "type"), ("an array", b"RXBc" + struct.pack("<I", 1) + b"\x01", "type"),
                            ("a byte left over", b"XaAq\x01", "walked"), ("an unknown type", b"Xa?" + b"\x01\x02\x03\x04", "walked"),
                            ("a value without its NUL", b"XaZabc", "walked"), ("an array beyond the record", b"XaBi" + struct.pack("<I", 1000), "walked")):
        bad = join([good, good, [with_aux(p[0], aux), p[1]]])
        for call in (lambda: bam_markdup(bad, host=True, barcode_tag="RX"), lambda: bam_dup_barcodes(bad, host=True, tag="RX"),
                     lambda: bam_sorted_file("@HD\tVN:1.6\n", CONTIGS, bad, host=True, markdup=True, barcode_tag="RX")):
            with pytest.raises(ValueError, match="record 4 .*" + word):
                call()
        bam_markdup(bad, host=True, barcode_name=True)                  # (name mode walks no tags)
        bam_markdup(join([good, good, [p[0], with_aux(p[1], aux)]]), host=True, barcode_tag="RX")      # (only a template's first record is read)


def test_command_refusals(capsys):
    from bwamem_hip import mem
    for argv, word in ((["--sort", "--barcode-tag", "RX", "-C", "idx", "r.fq"], "--markdup"), (["--sort", "--barcode-name", "idx", "r.fq"], "--markdup"),
                       (["--sort", "--markdup", "--barcode-tag", "RX", "idx", "r.fq"], "-C"), (["--sort", "--markdup", "-C", "--barcode-tag", "RG", "idx", "r.fq"], "RG"),
                       (["--sort", "--markdup", "-C", "--barcode-tag", "R", "idx", "r.fq"], "two characters"),
                       (["--sort", "--markdup", "-C", "--barcode-tag", "RX", "--barcode-name", "idx", "r.fq"], "one"), (["--sort", "--markdup", "-C", "idx", "r.fq", "--barcode-tag"], "--barcode-tag")):
        assert mem.main(argv) == 2, argv
        assert word in capsys.readouterr().err, argv
    assert "--barcode-tag" in mem.__doc__ and "--barcode-name" in mem.__doc__ and "know no UMI" not in mem.__doc__


# ---------------------------------------------------------------------------------------------------------------- the host forms under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_dup_umi_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_dup_umi_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_dup_core.h", "bam_dup.h", "bam_dup_host.cpp", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def test_host_forms_under_sanitizers(tmp_path):
    rng = np.random.default_rng(4)
    values = [b"", b"A", b"ACGT", LONG_A, LONG_B] + [bytes(rng.integers(0, 256, int(rng.integers(0, 70)), dtype=np.uint8).tolist()) for _ in range(500)]
    names = [b"", b":", b"a", b"a:", b":a", b"a:b:c", b"M:7:FC:1:11:5:6:ACGT", b"::"] + [bytes(rng.choice(list(b"01:::ACGT-+"), size=int(rng.integers(0, 40))).tolist()) for _ in range(2000)]
    members = [(c[0], c[1], c[2]) for c in cases()] + [("corpus %s %s %s" % k, corpus_stream(k[0], k[1]), corpus_kw(*k)) for k in CORPUS]
    p0 = pair(b"b", 1, 100, 0, 1, 251, 1)
    refused = [("a tag of another type", join([upair(b"g", 100, 300, b"AC"), [with_aux(p0[0], b"RXc\x01"), p0[1]]]), dict(barcode_tag="RX"), "record 2 "),
               ("a cut tag", join([[with_aux(p0[0], b"XaZab"), p0[1]]]), dict(barcode_tag="RX"), "record 0 "),
               ("a short tail", join([[with_aux(p0[0], b"RX"), p0[1]]]), dict(barcode_tag="RX"), "record 0 ")]
    fi, fo = str(tmp_path / "umi_case.bin"), str(tmp_path / "umi_result.bin")
    with open(fi, "wb") as f:
        for blobs in (values, names):
            f.write(struct.pack("<I", len(blobs)) + b"".join(struct.pack("<I", len(n)) + n for n in blobs))
        f.write(struct.pack("<I", len(members) + len(refused)))
        for _what, stream, kw, *_r in members + refused:
            groups = kw.get("read_groups") or []
            libs = list(dict.fromkeys(g[1] for g in groups))
            D = kw.get("optical_distance")
            f.write(struct.pack("<I2sqII", 2 if kw.get("barcode_name") else 1, kw.get("barcode_tag", "\0\0").encode(), -1 if D is None else D, kw.get("optical_max_set") or 0, len(groups)))
            f.write(b"".join(struct.pack("<I", len(g[0])) + g[0] + struct.pack("<i", libs.index(g[1])) for g in groups))
            f.write(struct.pack("<Q", len(stream)) + stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    with open(fo, "rb") as f:
        res = f.read()
    p = 0
    for v in values:
        assert struct.unpack_from("<Q", res, p)[0] == fnv1a(v), v
        p += 8
    n_field = 0
    for n in names:
        a, cut = struct.unpack_from("<II", res, p); p += 8
        k = n.rfind(b":")
        assert (a, cut) == ((k + 1, k) if k >= 0 else (len(n) + 1, len(n))), n
        n_field += k >= 0
    assert 20 < n_field < len(names) - 20
    for what, stream, kw in members:
        rc, = struct.unpack_from("<i", res, p); p += 4
        assert rc == 0, what
        want, counts, strings = umi_model(stream, tag=kw.get("barcode_tag"), name=kw.get("barcode_name", False), read_groups=kw.get("read_groups"),
                                          optical_distance=kw.get("optical_distance"), optical_max_set=kw.get("optical_max_set"))
        nt, = struct.unpack_from("<I", res, p); p += 4
        assert list(struct.unpack_from("<%dQ" % nt, res, p)) == [fnv1a(s or b"") for s in strings], what
        p += 8 * nt
        got = dict(zip(COUNT_KEYS, struct.unpack_from("<8Q", res, p))); p += 64
        got["templates_without_barcode"], = struct.unpack_from("<Q", res, p); p += 8
        opt = struct.unpack_from("<3Q", res, p); p += 24
        if kw.get("optical_distance") is not None:
            got.update(zip(OPT_KEYS, opt))
        nl, = struct.unpack_from("<I", res, p); p += 4
        assert nl == (2 if kw.get("read_groups") else 0), what
        if nl:
            lc = struct.unpack_from("<%dQ" % (8 * nl), res, p); p += 64 * nl
            lo = struct.unpack_from("<%dQ" % (3 * nl), res, p); p += 24 * nl
            got["libraries"] = {}
            for k, lb in enumerate(("lib1", "lib2")):
                got["libraries"][lb] = dict(zip(COUNT_KEYS, lc[8 * k:8 * k + 8]))
                if kw.get("optical_distance") is not None:
                    got["libraries"][lb].update(zip(OPT_KEYS, lo[3 * k:3 * k + 3]))
        assert got == counts, what
        assert res[p:p + len(stream)] == want, what
        p += len(stream)
    for what, _stream, _kw, word in refused:
        rc, n = struct.unpack_from("<iI", res, p); p += 8
        assert rc == -2 and word in res[p:p + n].decode(), (what, res[p:p + n])
        p += n
    assert p == len(res)
