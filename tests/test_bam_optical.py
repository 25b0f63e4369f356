"""Optical duplicates and the library-size estimate of duplicate marking, host forms: the name parser, the templates' locations, the clustering
through bam_markdup(host=True, optical_distance=D), the metrics table and the command's refusals -- against a model written here from the rules: per set
brute-force pairwise edges and connected components by a search over them (no sort, no union-find: it shares no method with the code under test).  Every
hand-made case also spells out the count it must give.  tests/bam_dup_optical_host.cpp runs the same host forms as plain C++ under AddressSanitizer and UBSan.
The corpus runs on the device in test_bam_optical_gpu.py."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from test_bam_dup import end_word, flag_of, name_of, pair, rec, templates_of
from test_bam_sort import split_records
from test_read_groups import rg_of

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_SET = 300_000
LIBRARY_SIZES = [(1000, 900, 4660), (12, 7, 10), (1_000_000, 800_000, 2_154_184), (2, 1, 1), (500, 499, 124_833), (10, 10, None), (0, 0, None)]


# ---------------------------------------------------------------------------------------------------------------- records

def with_rg(r: bytes, rg: bytes) -> bytes:
    """the record with an RG:Z tag behind its qualities"""
    body = r[4:] + b"RGZ" + rg + b"\0"
    return struct.pack("<I", len(body)) + body


def opair(name, pos1, pos2, q=30, rg=None, swap=False, rid=1):
    """a pair with ends at pos1 (forward) and pos2 (reverse); swap: read 2 holds the forward (smaller) end"""
    p = pair(name, rid, pos2, 1, rid, pos1, 0, q=q) if swap else pair(name, rid, pos1, 0, rid, pos2, 1, q=q)
    return [with_rg(r, rg) for r in p] if rg is not None else p


def nm(tile, x, y, seven=True, k=0):
    return (b"M%d:7:FC:1:%d:%d:%d" if seven else b"F%d:1:%d:%d:%d") % (k, tile, x, y)


# ---------------------------------------------------------------------------------------------------------------- the model

def name_location(name: bytes):
    """(tile, x, y) by the rules, or None"""
    f = name.split(b":")
    if len(f) not in (5, 7):
        return None
    out = []
    for v in f[-3:]:
        k = 0
        while k < len(v) and 48 <= v[k] <= 57:
            k += 1
        if k == 0 or int(v[:k]) >= 1 << 31:
            return None
        out.append(int(v[:k]))
    return tuple(out)


def template_info(stream: bytes, read_groups=None):
    """per template: (is a pair, set key, role, rg row, location or None, library name)"""
    recs = split_records(stream)
    out = []
    for t in templates_of(recs):
        pri = [recs[i] for i in t if not flag_of(recs[i]) & 0x900]
        mapped = [p for p in pri if not flag_of(p) & 4]
        row, lib = 0, None
        if read_groups is not None:
            row = [g[0] if isinstance(g[0], bytes) else g[0].encode() for g in read_groups].index(rg_of(recs[t[0]]).encode())
            lib = read_groups[row][1]
        is_pair = bool(flag_of(pri[0]) & 1) and len(mapped) == 2
        key, role = None, 0
        if is_pair:
            w = [(end_word(p), flag_of(p) & 0x80) for p in mapped]
            lo = min(w)
            key = (lib, min(w[0][0], w[1][0]), max(w[0][0], w[1][0]))
            role = 1 if w[0][0] != w[1][0] and lo[1] else 0
        out.append((is_pair, key, role, row, name_location(name_of(recs[t[0]])), lib))
    return out


def optical_model(stream: bytes, D: int, max_set: int = MAX_SET, read_groups=None):
    """(the three counts, the same per library name, statistics: cluster sizes, clusters per examined set, sizes of the skipped sets)"""
    info = template_info(stream, read_groups)
    libs = list(dict.fromkeys(g[1] for g in read_groups)) if read_groups is not None else [None]
    per = {lb: dict(optical_duplicate_pairs=0, located_pairs=0, optical_sets_skipped=0) for lb in libs}
    sets = {}
    for is_pair, key, role, row, loc, lib in info:
        if is_pair:
            sets.setdefault(key, []).append((role, row, loc))
            per[lib]["located_pairs"] += loc is not None
    sizes, per_set, skipped = [], [], []
    for key, members in sets.items():
        if len(members) < 2:
            continue
        if len(members) > max_set:
            per[key[0]]["optical_sets_skipped"] += 1
            skipped.append(len(members))
            continue
        m = [v for v in members if v[2] is not None]
        edge = [[a != b and m[a][0] == m[b][0] and m[a][1] == m[b][1] and m[a][2][0] == m[b][2][0] and abs(m[a][2][1] - m[b][2][1]) <= D and abs(m[a][2][2] - m[b][2][2]) <= D
                 for b in range(len(m))] for a in range(len(m))]
        seen, comps = set(), 0
        for a in range(len(m)):
            if a in seen:
                continue
            comps += 1
            todo, size = [a], 0
            seen.add(a)
            while todo:
                v = todo.pop(); size += 1
                for b in range(len(m)):
                    if edge[v][b] and b not in seen:
                        seen.add(b); todo.append(b)
            sizes.append(size)
        per_set.append(comps)
        per[key[0]]["optical_duplicate_pairs"] += len(m) - comps
    total = {k: sum(p[k] for p in per.values()) for k in ("optical_duplicate_pairs", "located_pairs", "optical_sets_skipped")}
    return total, per, dict(sizes=sizes, per_set=per_set, skipped=skipped)


# ---------------------------------------------------------------------------------------------------------------- hand-made cases

GROUPS = [(b"laneA", "lib1"), (b"laneB", "lib1"), (b"other", "lib2")]


def cases():
    """[(what, stream, keywords of bam_markdup, optical duplicate pairs, located pairs, sets skipped)]"""
    D = 100
    out = []

    def add(what, recs, opt, loc, skipped=0, **kw):
        kw.setdefault("optical_distance", D)
        out.append((what, b"".join(r for t in recs for r in t), kw, opt, loc, skipped))
    for what, dx, dy, want in (("dx at D", D, 0, 1), ("dx at D + 1", D + 1, 0, 0), ("dy at D", 0, D, 1), ("dy at D + 1", 0, D + 1, 0), ("dx and dy at D", D, D, 1),
                               ("dx below, dy beyond", 3, D + 1, 0)):
        add(what, [opair(nm(1101, 1000, 1000), 100, 300), opair(nm(1101, 1000 + dx, 1000 - dy, k=1), 100, 300)], want, 2)
    add("D = 0, one place", [opair(nm(5, 7, 9), 100, 300), opair(nm(5, 7, 9, k=1), 100, 300)], 1, 2, optical_distance=0)
    add("D = 0, one pixel apart", [opair(nm(5, 7, 9), 100, 300), opair(nm(5, 8, 9, k=1), 100, 300)], 0, 2, optical_distance=0)
    add("the largest D", [opair(nm(5, 0, 0), 100, 300), opair(nm(5, 2147483647, 2147483647, k=1), 100, 300)], 1, 2, optical_distance=2147483647)
    add("five fields against seven", [opair(nm(1101, 10, 10, seven=False), 100, 300), opair(nm(1101, 20, 20), 100, 300)], 1, 2)
    add("another tile", [opair(nm(1101, 10, 10), 100, 300), opair(nm(1102, 10, 10, k=1), 100, 300)], 0, 2)
    add("another read group of the library", [opair(nm(1, 10, 10), 100, 300, rg=b"laneA"), opair(nm(1, 10, 10, k=1), 100, 300, rg=b"laneB")], 0, 2, read_groups=GROUPS)
    add("one read group", [opair(nm(1, 10, 10), 100, 300, rg=b"laneB"), opair(nm(1, 10, 10, k=1), 100, 300, rg=b"laneB")], 1, 2, read_groups=GROUPS)
    add("another library", [opair(nm(1, 10, 10), 100, 300, rg=b"laneA"), opair(nm(1, 10, 10, k=1), 100, 300, rg=b"other")], 0, 2, read_groups=GROUPS)
    add("another role", [opair(nm(1, 10, 10), 100, 300), opair(nm(1, 10, 10, k=1), 100, 300, swap=True)], 0, 2)
    add("one role, read 2 first", [opair(nm(1, 10, 10), 100, 300, swap=True), opair(nm(1, 10, 10, k=1), 100, 300, swap=True)], 1, 2)
    add("an unlocated member inside a cluster's reach", [opair(nm(1, 10, 10), 100, 300), opair(b"plain_name", 100, 300), opair(nm(1, 60, 10, k=1), 100, 300)], 1, 2)
    add("a chain a-b-c with |a - c| = 2 D", [opair(nm(1, 0, 50), 100, 300), opair(nm(1, 2 * D, 50, k=1), 100, 300), opair(nm(1, D, 50, k=2), 100, 300)], 2, 3)
    add("a chain along y", [opair(nm(1, 50, 0), 100, 300), opair(nm(1, 50, 2 * D, k=1), 100, 300), opair(nm(1, 50, D, k=2), 100, 300)], 2, 3)
    add("two clusters in one set", [opair(nm(1, 0, 0), 100, 300), opair(nm(1, 5000, 0, k=1), 100, 300), opair(nm(1, 50, 0, k=2), 100, 300), opair(nm(1, 5050, 0, k=3), 100, 300)], 2, 4)
    add("the kept pair outside every cluster", [opair(nm(1, 9000, 9000), 100, 300, q=40), opair(nm(1, 10, 10, k=1), 100, 300), opair(nm(1, 20, 20, k=2), 100, 300)], 1, 3)
    add("a fragment sharing an end", [opair(nm(1, 10, 10), 100, 300), [rec(nm(1, 12, 12, k=1), 1, 100, 0)], opair(nm(1, 5000, 10, k=2), 100, 300)], 0, 2)
    add("sets of one pair", [opair(nm(1, 10, 10), 100, 300), opair(nm(1, 10, 10, k=1), 1100, 1300)], 0, 2)
    add("a set of max_set", [opair(nm(1, 10 + k, 10, k=k), 100, 300) for k in range(8)], 7, 8, optical_max_set=8)
    add("a set of max_set + 1", [opair(nm(1, 10 + k, 10, k=k), 100, 300) for k in range(9)], 0, 9, 1, optical_max_set=8)
    add("no templates", [], 0, 0)
    return out


def random_corpus(seed=11, n=420):
    """a few hundred pairs over a handful of keys, three read groups of two libraries, both roles, a 3 x 400 x 400 location space, some names without a location;
    a third of the pairs are copies of an earlier pair of their key a few pixels away (what an optical duplicate is), the others lie anywhere; one key holds more
    pairs than the test's max_set (30)"""
    rng = np.random.default_rng(seed)
    recs, seen = [], {}
    for k in range(n):
        key = int(rng.integers(0, 8)) if k % 3 else int(rng.integers(8, 60))
        if k < 40:
            key = 60                                               # one set of 40 in one library: skipped at max_set = 30
        rg = b"other" if key == 60 else GROUPS[int(rng.integers(0, 3))][0]
        swap = bool(rng.integers(0, 4) == 0)
        tile, x, y = int(rng.integers(1, 4)), int(rng.integers(0, 400)), int(rng.integers(0, 400))
        if seen.get(key) and rng.integers(0, 3) == 0:
            rg, swap, tile, x, y = seen[key][int(rng.integers(0, len(seen[key])))]
            x, y = max(0, x + int(rng.integers(-20, 21))), max(0, y + int(rng.integers(-20, 21)))
        seen.setdefault(key, []).append((rg, swap, tile, x, y))
        name = b"noloc%d" % k if rng.integers(0, 12) == 0 else nm(tile, x, y, seven=bool(k & 1), k=k)
        recs.append(opair(name, 1000 + 10 * key, 1400 + 10 * key, q=int(rng.integers(20, 40)), rg=rg, swap=swap))
        if rng.integers(0, 10) == 0:
            recs.append([with_rg(rec(nm(1, int(rng.integers(0, 400)), 5, k=k + 1000), 1, 1000 + 10 * key, 0), rg)])
    return b"".join(r for t in recs for r in t)


CORPUS_KW = dict(read_groups=GROUPS, optical_distance=25, optical_max_set=30)


def model_counts(stream, kw):
    return optical_model(stream, kw["optical_distance"], kw.get("optical_max_set") or MAX_SET, kw.get("read_groups"))


def assert_equals_model(counts, stream, kw, what):
    total, per, _stats = model_counts(stream, kw)
    assert {k: counts[k] for k in total} == total, what
    if kw.get("read_groups") is not None:
        assert {lb: {k: c[k] for k in total} for lb, c in counts["libraries"].items()} == per, what


# ---------------------------------------------------------------------------------------------------------------- the tests

PARSER_TABLE = [
    (b"FC:1:1101:2104:15343", (1101, 2104, 15343)),               # 5 fields
    (b"M01:55:FC:1:1101:2104:15343", (1101, 2104, 15343)),        # 7 fields
    (b"1:1101:2104:15343", None),                                 # 4
    (b"A:FC:1:1101:2104:15343", None),                            # 6
    (b"X:M01:55:FC:1:1101:2104:15343", None),                     # 8
    (b"FC:1::2104:15343", None),                                  # an empty field
    (b"FC:1:1101:2104:", None),
    (b"FC:1:1101:x2104:15343", None),                             # a letter first
    (b"FC:1:1101:-5:15343", None),                                # a sign
    (b"FC:1:1101:+5:15343", None),
    (b"FC:1:1101:2104:15343#ACGT", (1101, 2104, 15343)),          # bytes behind the digits
    (b"FC:1:1101:2104:15343/1", (1101, 2104, 15343)),
    (b"FC:1:11a01:2104 x:15343", (11, 2104, 15343)),
    (b"FC:1:0:0:0", (0, 0, 0)),                                   # value 0
    (b"FC:1:007:00:0000000000000000000012", (7, 0, 12)),          # leading zeros are digits
    (b"FC:1:2147483647:2147483647:2147483647", (2147483647,) * 3),
    (b"FC:1:1:2147483648:1", None),                               # 2^31
    (b"FC:1:1:1:99999999999999999999999999", None),               # beyond 64 bits
    (b"", None), (b":", None), (b"::::", None), (b"::::::", None), (b"::1:2:3", (1, 2, 3)),
    (b"N" * 234 + b":1:12345:678901:2345", (12345, 678901, 2345)),     # 254 bytes, the longest name a record holds
]


def test_name_parser():
    from bwamem_hip.lib import bam_name_location
    assert len(PARSER_TABLE[-1][0]) == 254
    for name, want in PARSER_TABLE:
        assert name_location(name) == want, name                  # the model against the table
        assert bam_name_location(name) == want, name


def test_locations_host():
    from bwamem_hip.lib import bam_dup_locations
    groups = [(b"laneA", "lib1"), (b"laneB", "lib1")]
    recs = [opair(nm(1101, 5, 6), 100, 300, rg=b"laneA"),                          # read 1 holds the smaller end: role 0
            opair(nm(1102, 7, 8, seven=False), 100, 300, rg=b"laneB", swap=True),  # read 2 holds it: role 1; the second row
            [with_rg(r, b"laneB") for r in pair(nm(3, 9, 10), 1, 500, 0, 1, 500, 0)],      # both ends at one word: role 0
            opair(b"no_location", 100, 300, rg=b"laneA", swap=True),               # unlocated: the role is still there
            [with_rg(rec(nm(4, 1, 2), 1, 700, 0), b"laneB")],                      # a fragment has a location and no role
            [with_rg(rec(nm(4, 3, 4), -1, -1, 4, ops=()), b"laneA")]]              # so has an unmapped read
    stream = b"".join(r for t in recs for r in t)
    L = bam_dup_locations(stream, host=True, read_groups=groups)
    assert [tuple(int(v) for v in l) for l in L] == [(5, 6, 1101, 0, 1), (7, 8, 1102, 1, 3), (9, 10, 3, 1, 1), (0, 0, 0, 0, 2), (1, 2, 4, 1, 1), (3, 4, 4, 0, 1)]
    info = template_info(stream, groups)                          # the model's roles and rows agree
    assert [(i[2], i[3], i[4]) for i in info][:4] == [(0, 0, (1101, 5, 6)), (1, 1, (1102, 7, 8)), (0, 1, (3, 9, 10)), (1, 0, None)]
    # without read groups no tag is read and the row is 0
    plain = b"".join(r for t in (opair(nm(1, 2, 3), 100, 300), opair(nm(1, 2, 3), 100, 300, swap=True)) for r in t)
    assert [tuple(int(v) for v in l) for l in bam_dup_locations(plain, host=True)] == [(2, 3, 1, 0, 1), (2, 3, 1, 0, 3)]
    assert len(bam_dup_locations(b"", host=True)) == 0
    with pytest.raises(ValueError):
        bam_dup_locations(stream[:-3], host=True, read_groups=groups)
    with pytest.raises(ValueError):
        bam_dup_locations(stream, host=True, read_groups=groups[:1])          # laneB is not listed


@pytest.mark.parametrize("case", cases(), ids=[c[0] for c in cases()])
def test_hand_made_cases_host(case):
    from bwamem_hip.lib import bam_markdup
    what, stream, kw, opt, loc, skipped = case
    total, _per, _stats = model_counts(stream, kw)
    assert (total["optical_duplicate_pairs"], total["located_pairs"], total["optical_sets_skipped"]) == (opt, loc, skipped), what      # the model against the hand count
    out, counts = bam_markdup(stream, host=True, **kw)
    assert_equals_model(counts, stream, kw, what)
    base_kw = {k: v for k, v in kw.items() if not k.startswith("optical")}
    out0, counts0 = bam_markdup(stream, host=True, **base_kw)
    assert out == out0 and all(counts[k] == v for k, v in counts0.items() if k != "libraries"), what


def test_corpus_is_not_vacuous():
    total, per, stats = model_counts(random_corpus(), CORPUS_KW)
    assert max(stats["sizes"]) >= 3 and max(stats["per_set"]) >= 2 and stats["skipped"] and max(stats["skipped"]) > 30
    assert total["optical_duplicate_pairs"] > 10 and all(p["optical_duplicate_pairs"] > 0 for p in per.values()) and len(per) == 2
    assert total["located_pairs"] < sum(1 for i in template_info(random_corpus(), GROUPS) if i[0])           # some pairs have no location
    # closeness is transitive: some cluster holds two members that are no neighbours themselves -- the count differs from that of a rule without chains
    assert any(s >= 3 for s in stats["sizes"])


def test_corpus_host_equals_model():
    from bwamem_hip.lib import MARKDUP_COUNTS, bam_markdup
    stream = random_corpus()
    out, counts = bam_markdup(stream, host=True, **CORPUS_KW)
    assert_equals_model(counts, stream, CORPUS_KW, "corpus")
    out0, counts0 = bam_markdup(stream, host=True, read_groups=GROUPS)
    assert out == out0 and [counts[k] for k in MARKDUP_COUNTS] == [counts0[k] for k in MARKDUP_COUNTS]
    assert {lb: [c[k] for k in MARKDUP_COUNTS] for lb, c in counts["libraries"].items()} == {lb: [c[k] for k in MARKDUP_COUNTS] for lb, c in counts0["libraries"].items()}
    assert "optical_duplicate_pairs" not in counts0 and "optical_duplicate_pairs" not in counts0["libraries"]["lib1"]
    # the count does not hang on the order of the input
    recs = split_records(stream)
    tpls = templates_of(recs)
    order = np.random.default_rng(5).permutation(len(tpls))
    shuffled = b"".join(recs[i] for t in order for i in tpls[t])
    _o, c2 = bam_markdup(shuffled, host=True, **CORPUS_KW)
    assert {k: c2[k] for k in ("optical_duplicate_pairs", "located_pairs", "optical_sets_skipped")} == {k: counts[k] for k in ("optical_duplicate_pairs", "located_pairs", "optical_sets_skipped")}
    # with the default max_set nothing is skipped
    kw = dict(CORPUS_KW, optical_max_set=None)
    _o, c3 = bam_markdup(stream, host=True, **kw)
    assert c3["optical_sets_skipped"] == 0
    assert_equals_model(c3, stream, kw, "corpus, default max_set")


def test_keyword_refusals():
    from bwamem_hip.lib import bam_markdup
    stream = cases()[0][1]
    for kw in (dict(optical_distance=-1), dict(optical_distance=1 << 31), dict(optical_distance=1.5), dict(optical_distance=True), dict(optical_distance="100"),
               dict(optical_max_set=8), dict(optical_distance=10, optical_max_set=0), dict(optical_distance=10, optical_max_set=1 << 31)):
        with pytest.raises(ValueError):
            bam_markdup(stream, host=True, **kw)


def test_library_size():
    from bwamem_hip.lib import estimate_library_size
    for n, c, want in LIBRARY_SIZES:
        assert estimate_library_size(n, c) == want, (n, c)
    assert estimate_library_size(5, 9) is None and estimate_library_size(0, 3) is None


def test_metrics_text():
    from bwamem_hip.aligner import markdup_metrics_text, markdup_metrics_text_libraries
    counts = dict(pairs_examined=1010, fragments_examined=4, duplicate_pairs=110, duplicate_fragments=1, records_flagged=8, secondary_or_supplementary=2, unmapped_records=5, templates=20)
    today = markdup_metrics_text(counts, "@RG\tID:x\tLB:lib7")
    assert today.split("\n")[1].split("\t")[-2:] == ["READ_PAIR_DUPLICATES", "PERCENT_DUPLICATION"] and "OPTICAL" not in today and "ESTIMATED" not in today
    with_opt = dict(counts, optical_duplicate_pairs=10, located_pairs=1000, optical_sets_skipped=0)
    lines = markdup_metrics_text(with_opt, "@RG\tID:x\tLB:lib7").split("\n")
    assert lines[0] == today.split("\n")[0] and lines[3] == ""
    assert lines[1].split("\t") == ["LIBRARY", "UNPAIRED_READS_EXAMINED", "READ_PAIRS_EXAMINED", "SECONDARY_OR_SUPPLEMENTARY_RDS", "UNMAPPED_READS", "UNPAIRED_READ_DUPLICATES",
                                    "READ_PAIR_DUPLICATES", "READ_PAIR_OPTICAL_DUPLICATES", "PERCENT_DUPLICATION", "ESTIMATED_LIBRARY_SIZE"]
    row = dict(zip(lines[1].split("\t"), lines[2].split("\t")))
    assert row["LIBRARY"] == "lib7" and row["READ_PAIR_OPTICAL_DUPLICATES"] == "10" and row["ESTIMATED_LIBRARY_SIZE"] == "4660"        # n = 1000, c = 900
    assert row["PERCENT_DUPLICATION"] == today.split("\n")[2].split("\t")[-1]
    # nothing duplicated: the column is there and empty
    none = dict(with_opt, duplicate_pairs=0, optical_duplicate_pairs=0)
    assert markdup_metrics_text(none).split("\n")[2].split("\t")[-1] == "" and markdup_metrics_text(none).split("\n")[2].count("\t") == 9
    libs = markdup_metrics_text_libraries({"a": with_opt, "b": none}).split("\n")
    assert libs[1] == lines[1] and libs[2].split("\t")[-1] == "4660" and libs[3].split("\t")[-1] == "" and libs[4] == ""
    assert markdup_metrics_text_libraries({"a": counts}).split("\n")[1] == today.split("\n")[1]


def test_python_and_command_refusals(capsys):
    from bwamem_hip import mem
    from bwamem_hip.aligner import Aligner
    al = Aligner.__new__(Aligner)                                 # the keyword checks come before anything touches an index or a device
    al.profile = False
    for call in (lambda: al.align_file("r.fa", io.BytesIO(), fmt="bam", sort=True, optical_distance=100),                  # needs markdup
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, optical_distance=100),
                 lambda: al.align_files("r.fa", out=io.BytesIO(), optical_distance=100),
                 lambda: al.align_groups([("@RG\tID:a", "r.fa")], out=io.BytesIO(), fmt="bam", sort=True, optical_distance=100),
                 lambda: al.align_file("r.fa", io.BytesIO(), fmt="bam", sort=True, markdup=True, optical_distance=-1),
                 lambda: al.align_file("r.fa", io.BytesIO(), fmt="bam", sort=True, markdup=True, optical_distance=2.5),
                 lambda: al.align_files("r.fa", out=io.BytesIO(), fmt="bam", sort=True, markdup=True, optical_distance=1 << 31)):
        with pytest.raises(ValueError):
            call()
    assert getattr(al, "_out_fmt", ("sam", 1)) == ("sam", 1) and not getattr(al, "_markdup", False) and getattr(al, "_optical", None) is None
    assert mem.main(["--sort", "--optical-distance", "100", "prefix", "reads.fa"]) == 2
    assert "--optical-distance needs --markdup" in capsys.readouterr().err
    for bad in ("-5", "2.5", "abc", "", "2147483648"):
        assert mem.main(["--sort", "--markdup", "--optical-distance", bad, "prefix", "reads.fa"]) == 2, bad
        assert "--optical-distance needs a whole number" in capsys.readouterr().err
    assert mem.main(["--sort", "--markdup", "prefix", "reads.fa", "--optical-distance"]) == 2
    assert "--optical-distance" in mem.__doc__


# ---------------------------------------------------------------------------------------------------------------- the host forms under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_dup_optical_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_dup_optical_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_dup_core.h", "bam_dup.h", "bam_dup_host.cpp", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def test_host_forms_under_sanitizers(tmp_path):
    from bwamem_hip.lib import bam_dup_locations
    names = [n for n, _w in PARSER_TABLE]
    rng = np.random.default_rng(9)
    for _ in range(3000):                                         # generated names: digits, colons and what else a name may hold, of every length
        names.append(bytes(rng.choice(list(b"0123456789::::-+#a/ "), size=int(rng.integers(0, 40))).tolist()))
    members = [(c[0], c[1], c[2]) for c in cases()] + [("corpus", random_corpus(), CORPUS_KW), ("corpus, another seed", random_corpus(seed=3, n=300), dict(CORPUS_KW, optical_distance=60))]
    fi, fo = str(tmp_path / "opt_case.bin"), str(tmp_path / "opt_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(names)) + b"".join(struct.pack("<I", len(n)) + n for n in names))
        f.write(struct.pack("<I", len(members)))
        for _what, stream, kw in members:
            groups = kw.get("read_groups") or []
            libs = list(dict.fromkeys(g[1] for g in groups))
            f.write(struct.pack("<qII", kw["optical_distance"], kw.get("optical_max_set") or 0, len(groups)))
            f.write(b"".join(struct.pack("<I", len(g[0])) + g[0] + struct.pack("<i", libs.index(g[1])) for g in groups))
            f.write(struct.pack("<Q", len(stream)) + stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    with open(fo, "rb") as f:
        res = f.read()
    p = 0
    n_located = 0
    for n in names:
        ok, t, x, y = struct.unpack_from("<iIII", res, p); p += 16
        assert ((t, x, y) if ok else None) == name_location(n), n
        n_located += ok
    assert 20 < n_located < len(names) - 20                       # the generated names hold both kinds
    for what, stream, kw in members:
        rc, = struct.unpack_from("<i", res, p); p += 4
        assert rc == 0, what
        nt, = struct.unpack_from("<I", res, p); p += 4
        locs = res[p:p + 16 * nt]; p += 16 * nt
        assert locs == bam_dup_locations(stream, host=True, read_groups=kw.get("read_groups")).tobytes(), what
        p += 64
        opt = struct.unpack_from("<3Q", res, p); p += 24
        nl, = struct.unpack_from("<I", res, p); p += 4
        lib_opt = struct.unpack_from("<%dQ" % (3 * nl), res, p); p += 24 * nl
        total, per, _stats = model_counts(stream, kw)
        assert opt == (total["optical_duplicate_pairs"], total["located_pairs"], total["optical_sets_skipped"]), what
        assert [tuple(lib_opt[3 * k:3 * k + 3]) for k in range(nl)] == [(v["optical_duplicate_pairs"], v["located_pairs"], v["optical_sets_skipped"]) for v in per.values()][:nl] and nl == (len(per) if kw.get("read_groups") else 0), what
    assert p == len(res)
