"""Barcodes grouped within an edit distance (barcode_edits=N), host forms: bam_markdup(host=True, barcode_tag=... / barcode_name=True,
barcode_edits=N), bam_dup_barcodes(edits=True), barcode_pack, bam_sorted_file and the refusals -- against a brute-force model written here from the rules.  The
model groups the pairs by (library, end words) and the fragment pass's items by (library, end word), builds the components of each key's distinct barcode
*strings* by comparing every two of them position by position -- it never packs a value --, and applies test_bam_dup's rule (the best score stays, ties go to
the earlier template; a fragment goes where a pair has an end) per component.  The pair pass and the fragment pass are clustered independently.  Every hand-made
case also spells out the flags it must give.  All comparisons are exact.  tests/bam_dup_umi_edits_host.cpp runs the same host forms as plain C++ under
AddressSanitizer and UBSan.  The same cases run on the device in test_bam_umi_edits_gpu.py.

Every call passes barcode_edits= (or edits=), so every test raises TypeError on a tree without the feature."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from test_bam_dup import CONTIGS, end_word, flag_of, mask_dup, pair, score_of, set_dup, templates_of
from test_bam_optical import nm
from test_bam_sort import BamFile, check_file, split_records
from test_bam_umi import COUNT_KEYS, GROUPS, barcode_of, flags, join, render, rg_id, ufrag, upair, with_aux, z

HERE = os.path.dirname(os.path.abspath(__file__))
GROUP_KEYS = ("pair_barcodes_observed", "pair_barcodes_inferred", "barcode_keys_skipped")
SYMBOLS = {c: k + 1 for k, c in enumerate(b"ACGTN-+")}
CAP = 65536


# ---------------------------------------------------------------------------------------------------------------- the model

def near(a: bytes, b: bytes, N: int) -> bool:
    return len(a) == len(b) and sum(x != y for x, y in zip(a, b)) <= N


def components(strings, N: int, max_set: int):
    """({string: its component's label}, is the key over the cap): the connected components of the strings under `near`, by comparing every two of them"""
    strs = sorted(set(strings))
    if len(strs) > max_set:
        return {s: s for s in strs}, True
    label = {s: k for k, s in enumerate(strs)}
    changed = True
    while changed:                                                 # (labels flow along the edges until nothing moves: the components, in whatever order)
        changed = False
        for a in strs:
            for b in strs:
                if label[a] != label[b] and near(a, b, N):
                    label[a] = label[b] = min(label[a], label[b]); changed = True
    return label, False


def edits_model(stream: bytes, N: int, tag=None, name=False, read_groups=None, max_set=CAP):
    """(the records with 0x400 set, the counts as bam_markdup(barcode_edits=N) returns them, the barcode strings per template)"""
    recs = split_records(stream)
    tpls = templates_of(recs)
    lib_of = dict(read_groups) if read_groups is not None else {}
    libs = list(dict.fromkeys(lb for _id, lb in read_groups)) if read_groups is not None else [None]
    info = []                                                      # (library, barcode string, end words, score)
    for idx in tpls:
        first = recs[idx[0]]
        pri = [recs[i] for i in idx if not flag_of(recs[i]) & 0x900]
        words = tuple(sorted(end_word(p) for p in pri if not flag_of(p) & 4))
        info.append((lib_of[rg_id(first)] if read_groups is not None else None, barcode_of(first, tag, name), words, sum(score_of(p) for p in pri)))
    per = {lb: dict.fromkeys(COUNT_KEYS + GROUP_KEYS, 0) for lb in libs}
    dup = [False] * len(info)
    # the pair pass: per (library, lo, hi) the components of the pairs' distinct barcodes; per component the best pair stays
    keys = {}
    for o, (lb, bc, w, s) in enumerate(info):
        if len(w) == 2:
            keys.setdefault((lb, w), []).append(o)
    for (lb, _w), members in keys.items():
        label, over = components([info[o][1] for o in members if info[o][1] is not None], N, max_set)
        per[lb]["pair_barcodes_observed"] += len(label)
        per[lb]["pair_barcodes_inferred"] += len(set(label.values()))
        per[lb]["barcode_keys_skipped"] += over
        best = {}
        for o in members:
            c = label.get(info[o][1])                                # (None: no barcode -- such pairs are comparable with each other only)
            best[c] = min(best.get(c, (0, 1 << 40)), (-info[o][3], o))
        for o in members:
            dup[o] = best[label.get(info[o][1])][1] != o
    # the fragment pass: per (library, end word) the components of the items' distinct barcodes -- fragments and both ends of every pair, under their own barcodes
    ends = {}
    for o, (lb, bc, w, s) in enumerate(info):
        for word in w:
            ends.setdefault((lb, word), []).append(o)
    for (lb, _word), items in ends.items():
        label, over = components([info[o][1] for o in items if info[o][1] is not None], N, max_set)
        per[lb]["barcode_keys_skipped"] += over
        has_pair, best = set(), {}
        for o in items:
            c = label.get(info[o][1])
            if len(info[o][2]) == 2:
                has_pair.add(c)
            else:
                best[c] = min(best.get(c, (0, 1 << 40)), (-info[o][3], o))
        for o in items:
            c = label.get(info[o][1])
            if len(info[o][2]) == 1:
                dup[o] = c in has_pair or best[c][1] != o
    out = list(recs)
    for idx, d, (lb, bc, w, s) in zip(tpls, dup, info):
        p = per[lb]
        p["templates"] += 1
        p["pairs_examined"] += len(w) == 2
        p["fragments_examined"] += len(w) == 1
        p["duplicate_pairs"] += d and len(w) == 2
        p["duplicate_fragments"] += d and len(w) == 1
        p["records_flagged"] += len(idx) if d else 0
        p["secondary_or_supplementary"] += sum(1 for i in idx if flag_of(recs[i]) & 0x900)
        p["unmapped_records"] += sum(1 for i in idx if flag_of(recs[i]) & 4)
        if d:
            for i in idx:
                out[i] = set_dup(out[i])
    counts = {k: int(sum(per[lb][k] for lb in libs)) for k in COUNT_KEYS + GROUP_KEYS}
    counts["templates_without_barcode"] = sum(1 for i in info if i[1] is None)
    if read_groups is not None:
        counts["libraries"] = {lb: {k: int(v) for k, v in per[lb].items()} for lb in libs}
    return b"".join(out), counts, [i[1] for i in info]


def pack(v: bytes) -> int:
    """the hand table's packing: symbol i in bits 3 i .. 3 i + 2"""
    return sum(SYMBOLS[c] << 3 * i for i, c in enumerate(v))


def model_kw(kw: dict) -> dict:
    return dict(N=kw["barcode_edits"], tag=kw.get("barcode_tag"), name=kw.get("barcode_name", False), read_groups=kw.get("read_groups"), max_set=kw.get("barcode_max_set") or CAP)


# ---------------------------------------------------------------------------------------------------------------- hand-made cases

V21 = b"ACGTACGTACGTACGTACGTA"                                      # 21 symbols: the most a word holds
V21B = V21[:-1] + b"C"


def cases():
    """[(what, stream, keywords, the 0x400 bit of every record, (observed, inferred, skipped))] -- every bit written out by hand from the rules"""
    out = []

    def add(what, tpls, bits, grp, N=1, **kw):
        kw = dict(kw or dict(barcode_tag="RX"), barcode_edits=N)
        s = join(tpls)
        assert len(split_records(s)) == len(bits), what
        out.append((what, s, kw, bits, grp))
    P = lambda n, umi, q=30, **k: upair(n, 100, 300, umi, q=q, **k)
    add("distance 1 joins at N = 1", [P(b"a1", b"AAAA", 20), P(b"a2", b"AAAT")], [1, 1, 0, 0], (2, 1, 0))
    add("distance 2 does not at N = 1", [P(b"a1", b"AAAA", 20), P(b"a2", b"AATT")], [0, 0, 0, 0], (2, 2, 0))
    add("distance 2 joins at N = 2", [P(b"a1", b"AAAA", 20), P(b"a2", b"AATT")], [1, 1, 0, 0], (2, 1, 0), N=2)
    add("distance 3 does not at N = 2", [P(b"a1", b"AAAA", 20), P(b"a2", b"ATTT")], [0, 0, 0, 0], (2, 2, 0), N=2)
    add("distance 1 does not at N = 0", [P(b"a1", b"AAAA", 20), P(b"a2", b"AAAT"), P(b"a3", b"AAAA")], [1, 1, 0, 0, 0, 0], (2, 2, 0), N=0)
    add("a chain is one cluster", [P(b"a1", b"AAAA", 10), P(b"a2", b"ATTT", 40), P(b"a3", b"AATT", 30), P(b"a4", b"AAAT", 20)], [1, 1, 0, 0, 1, 1, 1, 1], (4, 1, 0))
    add("the chain's ends alone are not", [P(b"a1", b"AAAA", 10), P(b"a2", b"ATTT", 40)], [0, 0, 0, 0], (2, 2, 0))
    add("two lengths on one key", [P(b"a1", b"ACGT", 20), P(b"a2", b"ACGTA"), P(b"a3", b"ACG")], [0, 0, 0, 0, 0, 0], (3, 3, 0))
    add("two lengths at the largest N", [P(b"a1", b"ACGT", 20), P(b"a2", b"ACGTA"), P(b"a3", b"TTTT")], [1, 1, 0, 0, 0, 0], (3, 2, 0), N=21)
    add("N is a symbol", [P(b"a1", b"ACNT", 20), P(b"a2", b"ACGT"), P(b"a3", b"NNGT", 10)], [1, 1, 0, 0, 0, 0], (3, 2, 0))
    add("- and + are symbols", [P(b"a1", b"AC-GT", 20), P(b"a2", b"AC+GT"), P(b"a3", b"ACTGT", 10)], [1, 1, 0, 0, 1, 1], (3, 1, 0))
    add("a separator elsewhere is two edits", [P(b"a1", b"AC-GT", 20), P(b"a2", b"ACG-T")], [0, 0, 0, 0], (2, 2, 0))
    add("a dual barcode that differs in one half", [P(b"a1", b"ACGT-TTGA", 20), P(b"a2", b"ACGT-TTGC"), P(b"a3", b"ACGA-TTGC", 10)], [1, 1, 0, 0, 1, 1], (3, 1, 0))
    add("a dual barcode that differs in both halves", [P(b"a1", b"ACGT-TTGA", 20), P(b"a2", b"ACGA-TTGC")], [0, 0, 0, 0], (2, 2, 0))
    add("21 symbols", [P(b"a1", V21, 20), P(b"a2", V21B), P(b"a3", V21[:-1])], [1, 1, 0, 0, 0, 0], (3, 2, 0))
    add("templates without a barcode are left alone", [P(b"a1", None, 40), P(b"a2", b""), P(b"a3", b"AC"), P(b"a4", b"AT"), ufrag(b"f", 100, None), ufrag(b"g", 100, b"AG")],
        [0, 0, 1, 1, 0, 0, 1, 1, 1, 1], (2, 1, 0))
    add("equal barcodes at different keys", [upair(b"a1", 100, 300, b"AAAA"), upair(b"a2", 100, 301, b"AAAT")], [0, 0, 0, 0], (2, 2, 0))
    # the fragment pass
    add("a fragment goes through a pair's end one edit away", [P(b"p", b"AAAA"), ufrag(b"f", 100, b"AAAT", q=40)], [0, 0, 1], (1, 1, 0))
    add("a fragment stays when the pair is two away", [P(b"p", b"AAAA"), ufrag(b"f", 100, b"AATT", q=40)], [0, 0, 0], (1, 1, 0))
    add("a fragment at the pair's reverse end", [P(b"p", b"AAAA"), ufrag(b"f", 300, b"CAAA", rev=True), ufrag(b"g", 300, b"CCCA", rev=True)], [0, 0, 1, 0], (1, 1, 0))      # (CCAA would chain to the pair through CAAA)
    add("the best fragment of a joined cluster stays", [ufrag(b"f1", 100, b"AAAA", q=20), ufrag(b"f2", 100, b"AAAT", q=30), ufrag(b"f3", 100, b"AATT", q=25), ufrag(b"f4", 100, b"GGGG", q=10)],
        [1, 0, 1, 0], (0, 0, 0))
    add("a fragment chains to a pair's end through another fragment", [P(b"p", b"AAAA"), ufrag(b"f1", 100, b"AATT", q=40), ufrag(b"f2", 100, b"AAAT")], [0, 0, 1, 1], (1, 1, 0))
    add("a bridging fragment does not merge the pairs", [P(b"p1", b"AAAA", 20), P(b"p2", b"AATT"), ufrag(b"f", 100, b"AAAT", q=40)], [0, 0, 0, 0, 1], (2, 2, 0))
    add("pairs of two keys join at their common end for the fragments only",
        [upair(b"p1", 100, 300, b"AAAA"), upair(b"p2", 100, 400, b"AATT"), ufrag(b"f1", 100, b"AAAT"), ufrag(b"f2", 400, b"AATA", rev=True), ufrag(b"f3", 300, b"AATT", rev=True)],
        [0, 0, 0, 0, 1, 1, 0], (2, 2, 0))
    # libraries
    add("two libraries with one key do not join", [P(b"a1", b"AAAA", rg=b"laneA"), P(b"a2", b"AAAT", rg=b"other"), P(b"a3", b"AAAT", 10, rg=b"laneB"), ufrag(b"f", 100, b"AAAC", rg=b"other")],
        [0, 0, 0, 0, 1, 1, 1], (3, 2, 0), barcode_tag="RX", read_groups=GROUPS)
    # name mode
    add("the name's last field", [pair(b"M:1:5:6:ACGT", 1, 100, 0, 1, 251, 1, q=20), pair(b"M:1:5:6:ACGA", 1, 100, 0, 1, 251, 1), pair(b"M:1:9:9:TCGT+AA", 1, 100, 0, 1, 251, 1),
                                  pair(b"M:1:9:9:TCGA+AA", 1, 100, 0, 1, 251, 1, q=20)], [1, 1, 0, 0, 0, 0, 1, 1], (4, 2, 0), barcode_name=True)
    add("no templates", [], [], (0, 0, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------- the synthetic stream

POOL = (b"ACGTAC", b"TTGACA", b"GGATCC", b"CATGNA", b"AC-TGA", b"TG+CAT")


def reads(n=3000, seed=11, n_pos=36):
    """n logical templates on n_pos positions (test_bam_umi.render's fields): 6-symbol barcodes drawn from a pool of six, two thirds of them with one symbol
    replaced, some with a second -- so most keys hold chains --, now and then none; pairs (both roles), fragments and pairs with an unmapped mate; three read groups"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        u = bytearray(POOL[int(rng.integers(0, len(POOL)))])
        for _ in range(int(rng.choice((0, 1, 1, 2)))):
            u[int(rng.integers(0, 6))] = b"ACGT"[int(rng.integers(0, 4))]
        kind = float(rng.random())
        out.append(dict(kind="pair" if kind < 0.6 else "frag" if kind < 0.85 else "half", pos=1000 + 37 * int(rng.integers(0, n_pos)), q=int(rng.integers(15, 40)),
                        umi=bytes(u) if rng.integers(0, 12) else None, rg=GROUPS[int(rng.integers(0, 3))][0], swap=bool(rng.integers(0, 4) == 0),
                        loc=(int(rng.integers(1, 3)), int(rng.integers(0, 300)), int(rng.integers(0, 300))), k=k, seven=bool(k & 1)))
    return out


_STREAMS, _MODELS = {}, {}
CORPUS = [(m, g) for m in ("tag", "name") for g in (False, True)]


def corpus_stream(mode: str, groups: bool) -> bytes:
    if (mode, groups) not in _STREAMS:
        _STREAMS[(mode, groups)] = render(reads(), mode, groups)
    return _STREAMS[(mode, groups)]


def corpus_kw(mode: str, groups: bool, N: int = 1) -> dict:
    kw = dict(barcode_tag="RX") if mode == "tag" else dict(barcode_name=True)
    if groups:
        kw["read_groups"] = GROUPS
    kw["barcode_edits"] = N
    return kw


def corpus_expected(mode: str, groups: bool, N: int = 1):
    """the model's answer on a corpus member, computed once and shared"""
    if (mode, groups, N) not in _MODELS:
        _MODELS[(mode, groups, N)] = edits_model(corpus_stream(mode, groups), **model_kw(corpus_kw(mode, groups, N)))
    return _MODELS[(mode, groups, N)]


def one_key_stream(n_umis=5):
    """one (lo, hi) and its two ends under a chain of n_umis barcodes, each one edit from the next: a pair and a fragment per barcode, scores ascending"""
    chain = [b"A" * (8 - k) + b"T" * k for k in range(n_umis)]
    return join([upair(b"p%d" % k, 100, 300, u, q=15 + k) for k, u in enumerate(chain)] + [ufrag(b"f%d" % k, 100, u, q=15 + k) for k, u in enumerate(chain)]), chain


def sorted_file_stream() -> bytes:
    """the first 300 templates of the tagged corpus with read groups"""
    return render(reads()[:300], "tag", True)


def optical_stream():
    """three pairs of one key a few pixels apart: AAAA and AAAT one molecule at N = 1, GGGG another"""
    return join([with_aux(r, z(b"RX", u)) for r in pair(nm(1, x, y, k=k), 1, 100, 0, 1, 251, 1, q=q)] for k, (u, x, y, q) in enumerate(((b"AAAA", 10, 10, 30), (b"AAAT", 12, 14, 20), (b"GGGG", 11, 11, 25))))


# ---------------------------------------------------------------------------------------------------------------- the tests

def test_barcode_pack():
    from bwamem_hip.lib import barcode_pack
    table = {b"": 0, b"A": 1, b"C": 2, b"G": 3, b"T": 4, b"N": 5, b"-": 6, b"+": 7, b"AC": 1 | 2 << 3, b"CA": 2 | 1 << 3, b"ACGT": 1 | 2 << 3 | 3 << 6 | 4 << 9,
             b"T-+N": 4 | 6 << 3 | 7 << 6 | 5 << 9, V21: sum((1, 2, 3, 4)[i % 4] << 3 * i for i in range(21))}
    for v, w in table.items():
        assert barcode_pack(v) == w == pack(v), v
    assert barcode_pack("ACGT") == barcode_pack(b"ACGT") and barcode_pack(b"T" * 21) == pack(b"T" * 21) < 1 << 63
    assert len({barcode_pack(v) for v in (b"A", b"AA", b"AAA", b"C", b"AC", b"CA")}) == 6      # injective across lengths
    for bad in (b"acgt", b"ACGU", b"AC GT", b"ACGT\0", b"A" * 22, V21 + b"A", b"ac", b"*"):
        with pytest.raises(ValueError):
            barcode_pack(bad)


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_hand_made_cases_host(case):
    from bwamem_hip.lib import bam_markdup
    what, stream, kw, bits, grp = case
    got, c = bam_markdup(stream, host=True, **kw)
    assert flags(got) == bits, what
    assert tuple(c[k] for k in GROUP_KEYS) == grp, what
    want, counts, _s = edits_model(stream, **model_kw(kw))
    assert flags(want) == bits and tuple(counts[k] for k in GROUP_KEYS) == grp, what      # (the model is pinned by the same hand-written bits)
    assert got == want and c == counts, what


def test_two_libraries_counts():
    from bwamem_hip.lib import bam_markdup
    case = next(c for c in cases() if c[0].startswith("two libraries"))
    _got, c = bam_markdup(case[1], host=True, **case[2])
    assert [c["libraries"]["lib1"][k] for k in GROUP_KEYS] == [2, 1, 0] and [c["libraries"]["lib2"][k] for k in GROUP_KEYS] == [1, 1, 0]
    assert c["libraries"]["lib1"]["duplicate_pairs"] == 1 and c["libraries"]["lib2"]["duplicate_fragments"] == 1


@pytest.mark.parametrize("mode,groups", CORPUS)
def test_corpus_host_equals_model(mode, groups):
    from bwamem_hip.lib import bam_markdup
    stream, kw = corpus_stream(mode, groups), corpus_kw(mode, groups)
    want, counts, _strings = corpus_expected(mode, groups)
    got, c = bam_markdup(stream, host=True, **kw)
    assert c == counts
    assert got == want
    exact_kw = {k: v for k, v in kw.items() if k != "barcode_edits"}
    _e, ec = bam_markdup(stream, host=True, **exact_kw)
    plain_kw = {k: v for k, v in exact_kw.items() if not k.startswith("barcode")}
    _p, pc = bam_markdup(stream, host=True, **plain_kw)
    n = lambda d: d["duplicate_pairs"] + d["duplicate_fragments"]
    assert 0 < n(ec) < n(c) < n(pc), (n(ec), n(c), n(pc))              # grouping finds copies the exact comparison misses, and still rescues templates
    assert 0 < c["pair_barcodes_inferred"] < c["pair_barcodes_observed"] and c["barcode_keys_skipped"] == 0
    assert 0 < c["templates_without_barcode"] < c["templates"]


@pytest.mark.parametrize("mode,groups", CORPUS)
def test_no_edits_equal_the_exact_mode(mode, groups):
    """N = 0: flags and counts of barcode_tag / barcode_name alone, on a stream whose barcodes pack"""
    from bwamem_hip.lib import bam_markdup
    stream, kw = corpus_stream(mode, groups), corpus_kw(mode, groups, 0)
    got, c = bam_markdup(stream, host=True, **kw)
    exact, ec = bam_markdup(stream, host=True, **{k: v for k, v in kw.items() if k != "barcode_edits"})
    assert got == exact
    assert c["pair_barcodes_observed"] == c["pair_barcodes_inferred"] > 0 and c["barcode_keys_skipped"] == 0
    strip = lambda d: {k: ({lb: strip(v) for lb, v in v.items()} if k == "libraries" else v) for k, v in d.items() if k not in GROUP_KEYS}
    assert strip(c) == ec
    want, counts, _s = corpus_expected(mode, groups, 0)
    assert got == want and c == counts


@pytest.mark.parametrize("N", (2, 3, 21))
def test_corpus_at_other_distances(N):
    from bwamem_hip.lib import bam_markdup
    stream, kw = corpus_stream("tag", True), corpus_kw("tag", True, N)
    want, counts, _s = corpus_expected("tag", True, N)
    got, c = bam_markdup(stream, host=True, **kw)
    assert c == counts and got == want


def test_without_the_option_nothing_changes():
    from bwamem_hip.lib import bam_markdup
    s = corpus_stream("tag", True)
    for kw in (dict(), dict(read_groups=GROUPS), dict(barcode_tag="RX"), dict(barcode_tag="RX", read_groups=GROUPS, optical_distance=25)):
        a, b = bam_markdup(s, host=True, **kw), bam_markdup(s, host=True, barcode_edits=None, barcode_max_set=None, **kw)
        assert a == b and not set(GROUP_KEYS) & set(a[1])


@pytest.mark.parametrize("mode", ("tag", "name"))
def test_packed_words_host(mode):
    from bwamem_hip.lib import bam_dup_barcodes, barcode_pack
    s = corpus_stream(mode, True)
    _m, _c, strings = corpus_expected(mode, True)
    src = dict(tag="RX") if mode == "tag" else dict(name=True)
    got = bam_dup_barcodes(s, host=True, edits=True, **src)
    assert got.dtype == np.uint64 and got.tolist() == [pack(v or b"") for v in strings] == [barcode_pack(v or b"") for v in strings]
    assert got.tolist() != bam_dup_barcodes(s, host=True, **src).tolist()      # (without edits: the hashes)


def test_the_cap():
    """barcode_max_set at a key's distinct count, one above and one below: below, the key's words stay exact and the key is counted -- once in the pair pass and
    once at each of its two ends in the fragment pass"""
    from bwamem_hip.lib import bam_markdup
    s, chain = one_key_stream(5)
    exact, _ec = bam_markdup(s, host=True, barcode_tag="RX")
    assert sum(flags(exact)) == 5                                     # (exact: only every fragment under its pair)
    for cap, skipped in ((5, 0), (6, 0), (4, 3), (1, 3)):
        kw = dict(barcode_tag="RX", barcode_edits=1, barcode_max_set=cap)
        got, c = bam_markdup(s, host=True, **kw)
        want, counts, _s = edits_model(s, **model_kw(kw))
        assert got == want and c == counts, cap
        assert (c["pair_barcodes_observed"], c["pair_barcodes_inferred"], c["barcode_keys_skipped"]) == (5, 5 if skipped else 1, skipped), cap
        assert (got == exact) == bool(skipped), cap
        if not skipped:
            assert flags(got) == [1, 1] * 4 + [0, 0] + [1] * 5, cap      # the best pair of the one cluster stays, every fragment goes


@pytest.mark.parametrize("window", (0, 1, 7, 100))
def test_sorted_file_host(window):
    from bwamem_hip.lib import bam_sorted_file
    hdr = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:x\tLN:1\n"
    s = sorted_file_stream()
    want, counts, _strings = edits_model(s, 1, tag="RX", read_groups=GROUPS)
    bam, bai, c = bam_sorted_file(hdr, CONTIGS, s, 1, window, host=True, markdup=True, read_groups=GROUPS, barcode_tag="RX", barcode_edits=1)
    assert c == counts
    f = check_file(bam, bai, hdr, CONTIGS, want, ("barcode edits", window), n_regions=10)      # the sorted file of the records as the model flags them
    exact = bam_sorted_file(hdr, CONTIGS, s, 1, window, host=True, markdup=True, read_groups=GROUPS, barcode_tag="RX")
    assert mask_dup(f.stream) == mask_dup(BamFile(exact[0]).stream)
    assert c["duplicate_pairs"] > exact[2]["duplicate_pairs"] > 0 and "pair_barcodes_observed" not in exact[2]
    bam2, csi, c2 = bam_sorted_file(hdr, CONTIGS, s, 1, window, host=True, markdup=True, read_groups=GROUPS, barcode_tag="RX", barcode_edits=1, index_format="csi")
    assert bam2 == bam and c2 == c and csi != bai


def test_an_optical_set_follows_the_canonical_word():
    from bwamem_hip.lib import bam_markdup
    s = optical_stream()
    _g, c = bam_markdup(s, host=True, barcode_tag="RX", barcode_edits=1, optical_distance=10)
    assert (c["duplicate_pairs"], c["optical_duplicate_pairs"], c["located_pairs"]) == (1, 1, 3)      # AAAA and AAAT: one set of two, four pixels apart
    _g, c = bam_markdup(s, host=True, barcode_tag="RX", barcode_edits=0, optical_distance=10)
    assert (c["duplicate_pairs"], c["optical_duplicate_pairs"], c["located_pairs"]) == (0, 0, 3)      # three sets of one
    _g, c = bam_markdup(s, host=True, barcode_tag="RX", barcode_edits=4, optical_distance=10)
    assert (c["duplicate_pairs"], c["optical_duplicate_pairs"]) == (2, 2)                              # every barcode within four: one set of three
    _g, c = bam_markdup(s, host=True, barcode_tag="RX", barcode_edits=1, optical_distance=3)
    assert (c["duplicate_pairs"], c["optical_duplicate_pairs"]) == (1, 0)


def test_refusals():
    from bwamem_hip.lib import _err, bam_dup_barcodes, bam_markdup, bam_sorted_file, load_library
    s = join([upair(b"a1", 100, 300, b"AC"), upair(b"a2", 100, 300, b"AT")])
    hdr = "@HD\tVN:1.6\n"
    # before anything is written: no source, no marking, N outside 0 .. 21
    with pytest.raises(ValueError, match="barcode_tag or barcode_name"):
        bam_markdup(s, host=True, barcode_edits=1)
    with pytest.raises(ValueError, match="barcode_tag or barcode_name"):
        bam_sorted_file(hdr, CONTIGS, s, host=True, markdup=True, barcode_edits=1)
    with pytest.raises(ValueError, match="markdup"):
        bam_sorted_file(hdr, CONTIGS, s, host=True, barcode_tag="RX", barcode_edits=1)
    for bad in (-1, 22, 1000, 1.0, "1", True):
        with pytest.raises(ValueError, match="0 .. 21"):
            bam_markdup(s, host=True, barcode_tag="RX", barcode_edits=bad)
        with pytest.raises(ValueError, match="0 .. 21"):
            bam_sorted_file(hdr, CONTIGS, s, host=True, markdup=True, barcode_name=True, barcode_edits=bad)
    with pytest.raises(ValueError, match="barcode_edits"):
        bam_markdup(s, host=True, barcode_tag="RX", barcode_max_set=5)
    for bad in (0, -3, 1 << 31, 2.5):
        with pytest.raises(ValueError, match="barcode_max_set"):
            bam_markdup(s, host=True, barcode_tag="RX", barcode_edits=1, barcode_max_set=bad)
    # the library's own check, behind Python's
    L = load_library()
    from bwamem_hip.lib import MarkdupOpt, MarkdupCounts, _markdup_api
    _markdup_api(L)
    out, res = C.c_void_p(), MarkdupCounts()

    def call(mode, tag, n, cap=0, r=res):
        o = MarkdupOpt()
        L.bmh_markdup_opt_default(C.byref(o))
        o.barcode_mode, o.barcode_tag, o.barcode_edits, o.barcode_max_set = mode, tag or b"", n, cap
        return L.bmh_bam_markdup_host(s, len(s), C.byref(o), C.byref(out), C.byref(r) if r is not None else None)
    for mode, tag, n, cap in ((1, b"RX", 22, 0), (1, b"RX", -2, 0), (0, None, 1, 0), (0, b"RX", 0, 0), (1, b"RX", 1, 1 << 31)):
        assert call(mode, tag, n, cap) == -2, (mode, tag, n, cap)
        assert out.value is None and "barcode" in _err(L)
    assert call(1, b"RX", 1, 0, None) == -2 and out.value is None      # (a call without its counts record)
    assert call(1, b"RX", 1) == 0 and res.counts[2] == 1 and list(res.grouped) == [2, 1, 0]
    L.bmh_free.argtypes = [C.c_void_p]; L.bmh_free(out)
    assert call(1, b"RX", -1) == 0 and res.counts[2] == 0               # (-1: the exact comparison)
    L.bmh_free(out)
    # records: a value that does not pack -- by the index of the template's first record, after the templates before it
    good = upair(b"g", 100, 300, b"AC")
    p = pair(b"b", 1, 100, 0, 1, 251, 1)
    for what, value in (("22 symbols", V21 + b"A"), ("lower case", b"acgt"), ("one lower-case byte", b"ACgT"), ("another letter", b"ACGU"), ("a digit", b"ACG7"), ("a blank", b"AC GT"),
                        ("300 bytes", b"ACGT" * 75)):
        bad = join([good, good, [with_aux(p[0], z(b"RX", value)), p[1]]])
        for fn in (lambda: bam_markdup(bad, host=True, barcode_tag="RX", barcode_edits=1), lambda: bam_dup_barcodes(bad, host=True, tag="RX", edits=True),
                   lambda: bam_markdup(bad, host=True, barcode_tag="RX", barcode_edits=0, read_groups=None, optical_distance=5),
                   lambda: bam_sorted_file(hdr, CONTIGS, bad, host=True, markdup=True, barcode_tag="RX", barcode_edits=1)):
            with pytest.raises(ValueError, match="record 4 .*does not pack"):
                fn()
        bam_markdup(bad, host=True, barcode_tag="RX")                   # (the exact comparison takes any value)
        bam_markdup(join([good, good, [p[0], with_aux(p[1], z(b"RX", value))]]), host=True, barcode_tag="RX", barcode_edits=1)      # (only a template's first record is read)
        named = join([good, good, pair(b"M:1:2:3:" + value, 1, 100, 0, 1, 251, 1)]) if b":" not in value and len(value) < 200 else None
        if named:
            with pytest.raises(ValueError, match="record 4 .*does not pack"):
                bam_markdup(named, host=True, barcode_name=True, barcode_edits=1)
    ok, c = bam_markdup(join([good, good, [with_aux(p[0], z(b"RX", V21)), p[1]]]), host=True, barcode_tag="RX", barcode_edits=1)      # 21 symbols pack
    assert c["pair_barcodes_observed"] == 2 and c["duplicate_pairs"] == 1      # (one barcode at each of the two keys; the second `good` is a copy)
    # a tag of another type still comes first when it is the earlier record
    both = join([[with_aux(p[0], b"RXc\x01"), p[1]], [with_aux(p[0], z(b"RX", b"acgt")), p[1]]])
    with pytest.raises(ValueError, match="record 0 .*type"):
        bam_markdup(both, host=True, barcode_tag="RX", barcode_edits=1)


def test_command_refusals(capsys):
    from bwamem_hip import mem
    for argv, word in ((["--sort", "--markdup", "--barcode-edits", "1", "idx", "r.fq"], "--barcode-tag or --barcode-name"),
                       (["--sort", "--barcode-name", "--barcode-edits", "1", "idx", "r.fq"], "--markdup"), (["--barcode-edits", "1", "idx", "r.fq"], "--markdup"),
                       (["--sort", "--markdup", "--barcode-name", "--barcode-edits", "22", "idx", "r.fq"], "0 .. 21"),
                       (["--sort", "--markdup", "--barcode-name", "--barcode-edits", "-1", "idx", "r.fq"], "0 .. 21"),
                       (["--sort", "--markdup", "--barcode-name", "--barcode-edits", "one", "idx", "r.fq"], "0 .. 21"),
                       (["--sort", "--markdup", "--barcode-name", "idx", "r.fq", "--barcode-edits"], "--barcode-edits")):
        assert mem.main(argv) == 2, argv
        assert word in capsys.readouterr().err, argv
    assert "--barcode-edits" in mem.__doc__ and "is not built" not in mem.__doc__


# ---------------------------------------------------------------------------------------------------------------- the host forms under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_dup_umi_edits_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_dup_umi_edits_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_dup_core.h", "bam_dup.h", "bam_dup_host.cpp", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def test_host_forms_under_sanitizers(tmp_path):
    rng = np.random.default_rng(4)
    alphabet = list(b"ACGTN-+")
    values = [b"", b"A", b"ACGT", V21, V21 + b"A", b"acgt", b"ACGU", b"A" * 300] + [bytes(rng.choice(alphabet + list(b"acX "), size=int(rng.integers(0, 26))).tolist()) for _ in range(300)] \
        + [bytes(rng.choice(alphabet, size=int(rng.integers(0, 22))).tolist()) for _ in range(300)]
    twos = []
    for _ in range(600):
        a = bytearray(rng.choice(alphabet, size=int(rng.integers(1, 22))).tolist())
        b = bytearray(a)
        for _k in range(int(rng.integers(0, 5))):
            b[int(rng.integers(0, len(b)))] = alphabet[int(rng.integers(0, 7))]
        if rng.integers(0, 6) == 0:
            b = b[:-1] if rng.integers(0, 2) and len(b) > 1 else b + b"A"[:len(b) < 21]
        twos.append((bytes(a), bytes(b), int(rng.integers(0, 5))))
    twos += [(V21, V21B, 0), (V21, V21B, 1), (V21, V21, 0), (b"T" * 21, b"A" * 21, 20), (b"T" * 21, b"A" * 21, 21), (b"", b"", 0), (b"A", b"", 21), (b"acgt", b"ACGT", 4)]
    s5, _chain = one_key_stream(5)
    members = [(c[0], c[1], c[2]) for c in cases()] + [("corpus %s %s" % k, corpus_stream(*k), corpus_kw(*k)) for k in CORPUS] \
        + [("corpus at N = %d" % N, corpus_stream("tag", True), corpus_kw("tag", True, N)) for N in (0, 2)] \
        + [("the cap at %d" % cap, s5, dict(barcode_tag="RX", barcode_edits=1, barcode_max_set=cap)) for cap in (4, 5, 6)] \
        + [("with the optical step", optical_stream(), dict(barcode_tag="RX", barcode_edits=1, optical_distance=10))]
    p0 = pair(b"b", 1, 100, 0, 1, 251, 1)
    good = upair(b"g", 100, 300, b"AC")
    refused = [("22 symbols", join([good, [with_aux(p0[0], z(b"RX", V21 + b"A")), p0[1]]]), dict(barcode_tag="RX", barcode_edits=1), "record 2 "),
               ("lower case", join([[with_aux(p0[0], z(b"RX", b"acgt")), p0[1]]]), dict(barcode_tag="RX", barcode_edits=0), "record 0 "),
               ("a name's field that does not pack", join([good, good, pair(b"M:1:2:3:ACGX", 1, 100, 0, 1, 251, 1)]), dict(barcode_name=True, barcode_edits=1), "record 4 "),
               ("a tag of another type", join([good, [with_aux(p0[0], b"RXc\x01"), p0[1]]]), dict(barcode_tag="RX", barcode_edits=1), "record 2 "),
               ("edits beyond 21", join([good]), dict(barcode_tag="RX", barcode_edits=22), "0 .. 21"),
               ("a cap of 2^31", join([good]), dict(barcode_tag="RX", barcode_edits=1, barcode_max_set=1 << 31), "2^31")]
    fi, fo = str(tmp_path / "edits_case.bin"), str(tmp_path / "edits_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(values)) + b"".join(struct.pack("<I", len(v)) + v for v in values))
        f.write(struct.pack("<I", len(twos)) + b"".join(struct.pack("<I", len(a)) + a + struct.pack("<I", len(b)) + b + struct.pack("<I", N) for a, b, N in twos))
        f.write(struct.pack("<I", len(members) + len(refused)))
        for _what, stream, kw, *_r in members + refused:
            groups = kw.get("read_groups") or []
            libs = list(dict.fromkeys(g[1] for g in groups))
            D = kw.get("optical_distance")
            f.write(struct.pack("<I2siIqI", 2 if kw.get("barcode_name") else 1, kw.get("barcode_tag", "\0\0").encode(), kw["barcode_edits"], kw.get("barcode_max_set") or 0,
                                -1 if D is None else D, len(groups)))
            f.write(b"".join(struct.pack("<I", len(g[0])) + g[0] + struct.pack("<i", libs.index(g[1])) for g in groups))
            f.write(struct.pack("<Q", len(stream)) + stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    with open(fo, "rb") as f:
        res = f.read()
    p = 0
    packs = lambda v: len(v) <= 21 and all(c in SYMBOLS for c in v)
    n_ok = 0
    for v in values:
        ok, w = struct.unpack_from("<iQ", res, p); p += 12
        assert ok == packs(v) and w == (pack(v) if ok else 0), v
        n_ok += ok
    assert 100 < n_ok < len(values) - 100
    n_near = 0
    for a, b, N in twos:
        got, = struct.unpack_from("<i", res, p); p += 4
        assert got == (near(a, b, N) if packs(a) and packs(b) else -1), (a, b, N)
        n_near += got == 1
    assert 100 < n_near < len(twos) - 100
    for what, stream, kw in members:
        rc, = struct.unpack_from("<i", res, p); p += 4
        assert rc == 0, what
        want, counts, strings = edits_model(stream, **model_kw(kw))
        nt, = struct.unpack_from("<I", res, p); p += 4
        assert list(struct.unpack_from("<%dQ" % nt, res, p)) == [pack(s or b"") for s in strings], what
        p += 8 * nt
        got = dict(zip(COUNT_KEYS, struct.unpack_from("<8Q", res, p))); p += 64
        got["templates_without_barcode"], = struct.unpack_from("<Q", res, p); p += 8
        got.update(zip(GROUP_KEYS, struct.unpack_from("<3Q", res, p))); p += 24
        opt = struct.unpack_from("<3Q", res, p); p += 24
        if kw.get("optical_distance") is not None:
            assert opt == (1, 3, 0), what
        nl, = struct.unpack_from("<I", res, p); p += 4
        assert nl == (2 if kw.get("read_groups") else 0), what
        if nl:
            lc = struct.unpack_from("<%dQ" % (8 * nl), res, p); p += 64 * nl
            lg = struct.unpack_from("<%dQ" % (3 * nl), res, p); p += 24 * nl
            got["libraries"] = {lb: dict(zip(COUNT_KEYS + GROUP_KEYS, lc[8 * k:8 * k + 8] + lg[3 * k:3 * k + 3])) for k, lb in enumerate(("lib1", "lib2"))}
        assert got == counts, what
        assert res[p:p + len(stream)] == want, what
        p += len(stream)
    for what, _stream, _kw, word in refused:
        rc, n = struct.unpack_from("<iI", res, p); p += 8
        assert rc == -2 and word in res[p:p + n].decode(), (what, res[p:p + n])
        p += n
    assert p == len(res)
