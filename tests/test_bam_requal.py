"""Applying a recalibration table to the base qualities on the host: qualities listed by hand, the library's tables and records against the
Python model (tests/requal_model.py), every refusal, the windows of the host merge, the appended members of the records, the report, and the core under the
sanitizers."""
import ctypes as C
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from recal_model import E_CUT, E_RG_ID, E_RG_NONE, E_RG_TYPE, E_TAGS, M, S, equal, genome, rrec, synth_records
from requal_model import (BASES, CAPPED, CHANGED, LOW, NOCTX, NOQUAL, REWRITTEN, SEEN, UNCHANGED, WORDS, apply_model, deltas, empty_table, put, random_table, same_counts, slot, split)

HERE = os.path.dirname(os.path.abspath(__file__))
AA, AC, CC, CG, NONE = 0, 1, 5, 6, 16
HUGE = 3_000_000_000      # observations without an error: an empirical quality at the cap of 93


def host(recs, table):
    from bwamem_hip.lib import bam_apply_recal
    out, counts = bam_apply_recal(b"".join(recs) if isinstance(recs, list) else recs, table, host=True)
    return split(out), counts


def quals(rec: bytes) -> list:
    l_name, n_ops, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    at = 36 + l_name + 4 * n_ops + (l_seq + 1) // 2
    return list(rec[at:at + l_seq])


def only_qualities_differ(before: bytes, after: bytes) -> bool:
    if len(before) != len(after):
        return False
    l_name, n_ops, l_seq = before[12], struct.unpack_from("<H", before, 16)[0], struct.unpack_from("<I", before, 20)[0]
    at = 36 + l_name + 4 * n_ops + (l_seq + 1) // 2
    return before[:at] == after[:at] and before[at + l_seq:] == after[at + l_seq:]


def read(seq, qual, flag=0, name=b"r", tag=b""):
    return rrec(name, 0, 0, flag, 30, ((len(seq), M),) if seq else (), seq, qual, tag)


def hand_table() -> dict:
    """count pairs whose empirical quality is a whole number: (8, 0) 10, (98, 0) 20, (998, 0) 30, (9998, 0) 40, (98, 9) 10, (998, 9) 20"""
    t = empty_table(max_cycle=5)
    # quality 30: 9998 observations, no error -> B = 40.  Cycles 1, 2, 3 at 10, 20, 30; contexts AA, AC, CG at 10, 20, 30; the rest where no read below comes
    put(t, 30, 1, AA, 8, 0); put(t, 30, 2, AC, 98, 0); put(t, 30, 3, CG, 998, 0); put(t, 30, -5, NONE, 8894, 0)
    # quality 31: the same over the cycles of a second read, no context observed
    put(t, 31, -1, NONE, 8, 0); put(t, 31, -2, NONE, 98, 0); put(t, 31, -3, NONE, 998, 0); put(t, 31, 5, NONE, 8894, 0)
    # quality 20: 998 observations, 9 errors -> B = 20; cycle 1 and context AA at 10
    put(t, 20, 1, AA, 98, 9); put(t, 20, -5, NONE, 900, 0)
    # quality 40: B about 84.8; cycle 1 and context AA at 10, cycle 2 and context CC at 93
    put(t, 40, 1, AA, 98, 9); put(t, 40, 2, CC, HUGE, 0)
    # qualities 10 and 11: one row each whose 256 B is 19 x 256 + 128 (rint of 4991.9988) and 39 x 256 + 127 (rint of 10111.0004): a fraction of .5 rounds up
    put(t, 10, 1, NONE, 711, 7); put(t, 11, 1, NONE, 17807, 1)
    return t


def delta_table() -> dict:
    """one observed quality: 998 observations of quality 30 with 9 errors -> the group's empirical quality is 20, its reported one 30, its delta -10"""
    t = empty_table()
    put(t, 30, 1, NONE, 998, 9)
    return t


HAND = [  # (what, the read, the qualities expected)
    ("forward", read("ACGT", 30), [10, 1, 20, 40]),                      # 40-30; 40-20-20 -> 0, clamped at 1; 40-10-10; cycle 4 and context GT without observations
    ("reverse", read("CGT", 30, 0x10), [20, 1, 10]),                     # read by the machine as ACG, last stored base first
    ("second of pair", read("ACGT", 31, 0x81), [10, 20, 30, 40]),        # cycles -1 .. -4
    ("second of pair, reverse", read("ACGT", 31, 0x91), [40, 30, 20, 10]),
    ("0x80 without 0x1", read("ACGT", 31, 0x80), [40, 40, 40, 40]),      # positive cycles: none observed at quality 31 but cycle 5
    ("no context in front", read("AA", 20), [10, 10]),                   # base 0: cycle 1 alone; base 1: cycle 2 unobserved, context AA
    ("an N", read("ANA", 30), [10, 20, 30]),                             # N: its cycle, no context; the base behind it: no context either
    ("clamped at 93", read("CCA", 40), [10, 93, 85]),                    # B + (10 - B); B + 2 (93 - B) = 101.2; B alone = 84.8
    ("a fraction of .5", read("A", 10), [20]),
    ("a fraction below .5", read("A", 11), [39]),
    ("below min_qual", read("ACGT", [0, 5, 30, 5]), [0, 5, 20, 5]),      # base 2: cycle 3, context CG
    ("never observed quality", read("ACGT", 33), [33, 33, 33, 33]),      # q + the group's delta; this table's is computed below
]


def test_the_qualities_listed_by_hand():
    from bwamem_hip.lib import recal_apply_tables
    t = hand_table()
    tabs = recal_apply_tables(t)
    assert np.array_equal(tabs, deltas(t))                                               # exact on the hand tables
    assert tabs[0, 30, 0] == 40 * 256 and tabs[0, 30, 1 + slot(1, 5)] == -30 * 256 and tabs[0, 30, 1 + 10 + AC] == -20 * 256 and tabs[0, 30, 1 + slot(4, 5)] == 0
    assert tabs[0, 10, 0] == 19 * 256 + 128 and tabs[0, 11, 0] == 39 * 256 + 127
    dg = tabs[0, 33, 0] - 33 * 256                                                        # (the group's delta, the same for every quality that was never observed)
    assert dg == tabs[0, 50, 0] - 50 * 256 and dg != 0
    for what, rec, want in HAND:
        got, _c = host([rec], t)
        if what == "never observed quality":
            want = [min(93, max(1, (33 * 256 + int(dg) + 128) >> 8))] * 4
        assert quals(got[0]) == want, what
        assert only_qualities_differ(rec, got[0]), what
    # the group's delta by hand: empirical 20, reported 30
    d = delta_table()
    got, c = host([read("ACGT", [30, 25, 93, 6]), read("AC", [94, 255]), read("ACG", [5, 0, 7])], d)
    assert [quals(r) for r in got] == [[20, 15, 83, 1], [83, 83], [5, 0, 1]]
    assert c["records_rewritten"] == 3 and c["bases_below_min_qual"] == 2 and c["bases_seen"] == 9 and c["bases_changed"] == 7 and c["bases_unchanged"] == 0
    assert c["qual_hist"][0][93] == 3 and c["qual_hist"][1][83] == 3 and c["qual_hist"][0][5] == c["qual_hist"][1][5] == 1 and c["bases_without_context"] == 2      # (the first base of the third read lies below min_qual: it is counted there alone)


def test_the_tables_and_the_records_against_the_model():
    from bwamem_hip.lib import recal_apply_tables
    contigs, ref, _pac, _hole = genome()
    differ = 0
    for seed, groups, cap in ((3, None, 500), (4, ["lane1", "lane2", "x"], 60), (5, None, 7)):
        t = random_table(seed, groups, max_cycle=cap)
        tabs, mine = recal_apply_tables(t), deltas(t)
        d = np.abs(tabs.astype(np.int64) - mine)
        assert tabs.shape == mine.shape and d.max() <= 1                                  # (a tie of rint over two log10 implementations may fall either way)
        differ += int((d > 0).sum())
        recs = synth_records(400, contigs, ref, seed=seed, groups=groups)
        want, wc = apply_model(recs, t, tabs)                                             # the model on the library's integers: exact
        got, c = host(recs, t)
        assert got == want and same_counts(c, wc)
        assert all(only_qualities_differ(a, b) for a, b in zip(recs, got))
        s = c["summary"]
        assert s[SEEN] == 400 and s[REWRITTEN] + s[NOQUAL] == 400 and s[LOW] + s[CHANGED] + s[UNCHANGED] == s[BASES] and s[CHANGED] > 1000 and s[NOCTX] >= s[REWRITTEN]
        assert c["qual_hist"][0].sum() == c["qual_hist"][1].sum() == s[BASES]
    print("table entries that differ from the model's by one unit:", differ)


def test_the_edges_of_a_record():
    t = random_table(6)
    recs = [read("", None), read("A", 40), read("ACGTA", 37), read("ACGT", None), read("ACG", [0xff, 0xff, 30]), read("ACGTAC", [0, 5, 6, 93, 94, 255]),
            rrec(b"u", -1, -1, 0x4 | 0x400 | 0x100 | 0x800, 0, (), "ACGTT", 25), rrec(b"clipped", 0, 5, 0, 30, ((2, S), (3, M), (1, S)), "ACGTAC", 25)]
    want, wc = apply_model(recs, t)
    got, c = host(recs, t)
    assert got == want and same_counts(c, wc) and c["records_without_qualities"] == 2 and c["records_rewritten"] == 6
    assert got[0] == recs[0] and got[3] == recs[3] and quals(got[4])[:2] != [0xff, 0xff] and quals(got[5])[:2] == [0, 5]
    assert quals(got[6]) != quals(recs[6]) and quals(got[7])[0] != 25                    # whatever the flags; clips are not removed: the first stored base is cycle 1


@pytest.mark.parametrize("cap", (1, 2, 500))
def test_cycles_around_the_cap(cap):
    t = random_table(7 + cap, max_cycle=cap, cycles=cap)
    rng = np.random.default_rng(cap)
    recs = []
    for n in (cap - 1, cap, cap + 1):
        if n < 1:
            continue
        seq = "".join("ACGT"[k] for k in rng.integers(0, 4, n))
        recs += [read(seq, [int(q) for q in rng.choice([6, 25, 40], n)], flag) for flag in (0, 0x10, 0x81, 0x91)]
    want, wc = apply_model(recs, t)
    got, c = host(recs, t)
    assert got == want and same_counts(c, wc) and c["cycles_capped"] > 0
    if cap == 1:                                                                          # every base of either sign shares the one cycle of its sign
        assert wc["summary"][CAPPED] == 4


def test_every_refusal_word_for_word_and_the_smallest_index():
    from bwamem_hip.lib import bam_apply_recal
    ids = ["lane1", "lane2"]
    t = random_table(8, ids, max_cycle=20, cycles=20)
    ok = read("ACGT", 30, tag=b"RGZlane2\0")
    bad = {E_TAGS: read("ACGT", 30, tag=b"RGZlane1"), E_RG_NONE: read("ACGT", 30, tag=b"NMC\x01"), E_RG_TYPE: read("ACGT", 30, tag=b"RGA1"), E_RG_ID: read("ACGT", 30, tag=b"RGZlane3\0"),
           E_CUT: (lambda r: r[:20] + struct.pack("<I", 40) + r[24:])(read("ACGT", 30, tag=b"RGZlane1\0"))}
    for code, rec in bad.items():
        assert apply_model([ok, ok, rec, ok], t) == ("refused", 2, code)
        with pytest.raises(ValueError) as e:
            bam_apply_recal(ok + ok + rec + ok, t, host=True)
        assert str(e.value) == "bmh_bam_requal: bmh_bam_requal_host: record 2 " + WORDS[code], code
    with pytest.raises(ValueError, match="record 1 has no RG tag"):                       # the smallest index, whatever follows
        bam_apply_recal(ok + bad[E_RG_NONE] + bad[E_RG_ID] + bad[E_TAGS], t, host=True)
    # a record without qualities is passed over before its tags are read; a table of the one group `*` reads no tags at all
    got, c = host([ok, read("ACGT", None, tag=b"RGZlane3\0")], t)
    assert c["records_without_qualities"] == 1
    got, c = host([bad[E_TAGS], bad[E_RG_ID]], random_table(8, None, max_cycle=20, cycles=20))
    assert c["records_rewritten"] == 2


def test_the_table_is_checked_before_anything_is_written():
    from bwamem_hip.lib import bam_apply_recal, recal_apply_tables
    rec = read("ACGT", 30)
    for change, words in ((lambda t: t["cycle_m"].__setitem__((0, 30, slot(2, 5), 1), 99), "holds 99 errors among 98 observations (group *, quality 30, cycle 2)"),
                          (lambda t: t["context_m"].__setitem__((0, 20, AA, 1), 99), "holds 99 errors among 98 observations (group *, quality 20, context 0)"),
                          (lambda t: t["cycle_m"].__setitem__((0, 31, slot(-1, 5), 0), 9), "counts 9999 observations and 0 errors by cycle, 9998 and 0 by context (group *, quality 31)"),
                          (lambda t: t["context_m"].__setitem__((0, 20, NONE, 1), 1), "counts 998 observations and 9 errors by cycle, 998 and 10 by context (group *, quality 20)"),
                          (lambda t: t.__setitem__("min_qual", 94), "min_qual 94 (0 .. 93)"), (lambda t: t.__setitem__("min_qual", -1), "min_qual -1 (0 .. 93)")):
        t = hand_table()
        change(t)
        for call in (lambda: bam_apply_recal(rec, t, host=True), lambda: recal_apply_tables(t)):
            with pytest.raises(ValueError) as e:
                call()
            assert words in str(e.value), words
    t = hand_table(); t["max_cycle"] = 0
    with pytest.raises(ValueError):
        recal_apply_tables(t)
    with pytest.raises(ValueError, match="read groups"):
        recal_apply_tables(dict(hand_table(), read_groups=["a", "b"]))
    with pytest.raises(ValueError, match="twice"):
        recal_apply_tables(random_table(1, ["a", "a"], max_cycle=3, cycles=3))


# ---------------------------------------------------------------------------------------------------------------- the windows of the host merge

@pytest.fixture(scope="module")
def G():
    contigs, ref, pac, _hole = genome()
    recs = synth_records(120, contigs, ref)
    recs = [r[:18] + bytes([r[18] & 0x14, r[19] & 0x6]) + r[20:] for r in recs[:80] if r[7] < 0x80]      # (single primary reads on a contig: marking takes every name as one template)
    recs += [r[:36] + b"z" + r[37:] for r in recs[:6]]                                    # (duplicates under other names)
    return dict(contigs=contigs, ref=ref, pac=pac, recs=recs, stream=b"".join(recs), table=random_table(9))


@pytest.mark.parametrize("window", (0, 1, 7, 25))
def test_the_windows_of_the_host_merge(G, window, tmp_path):
    from test_bam_sort import BamFile
    from bwamem_hip.bam import bam_post_file
    from bwamem_hip.lib import bam_recal, bam_sorted_file
    t = G["table"]
    for markdup in (False, True):
        plain = bam_sorted_file("@CO\tx\n", G["contigs"], G["stream"], 1, window, host=True, markdup=markdup)
        assert plain == bam_sorted_file("@CO\tx\n", G["contigs"], G["stream"], 1, window, host=True, markdup=markdup, apply_recal=None)      # off: nothing changes
        got = bam_sorted_file("@CO\tx\n", G["contigs"], G["stream"], 1, window, host=True, markdup=markdup, apply_recal=t)
        want, wc = apply_model(BamFile(plain[0]).stream, t)
        assert BamFile(got[0]).stream == b"".join(want) and same_counts(got[-1]["apply"], wc) and list(got[-1]) == ["apply"]
        if markdup:
            assert got[2] == plain[2] and any(r[19] & 0x4 for r in BamFile(got[0]).recs)   # marking chose on the original qualities
        # with recal beside it: the "after" table, of the qualities as written
        kw = dict(pac=G["pac"], l_pac=len(G["ref"]))
        both = bam_sorted_file("@CO\tx\n", G["contigs"], G["stream"], 1, window, host=True, markdup=markdup, apply_recal=t, recal=kw)
        assert both[0] == got[0] and equal(both[-1], bam_recal(BamFile(got[0]).stream, G["contigs"], G["pac"], len(G["ref"]), host=True)) and same_counts(both[-1]["apply"], wc)
        before = bam_sorted_file("@CO\tx\n", G["contigs"], G["stream"], 1, window, host=True, markdup=markdup, recal=kw)
        assert not equal(both[-1], before[-1]) and "apply" not in before[-1] and before[:-1] == plain
    # the stand-alone post-processing of a file takes the same option, without a reference
    src = tmp_path / "in.bam"
    src.write_bytes(bam_sorted_file("@HD\tVN:1.6\tSO:unsorted\n", G["contigs"], G["stream"], 1, 0, host=True)[0])
    out, rep = io.BytesIO(), io.StringIO()
    r = bam_post_file(str(src), out, host=True, sort_window=window, markdup=True, apply_recal=t, apply_recal_report=rep)
    assert BamFile(out.getvalue()).stream == BamFile(got[0]).stream and same_counts(r["recal_apply"], wc)
    assert rep.getvalue().startswith("AS\trecords_seen\t%d\n" % len(G["recs"]))
    empty = bam_sorted_file("@CO\tx\n", G["contigs"], b"", 1, window, host=True, apply_recal=t)
    assert empty[-1]["apply"]["records_seen"] == 0 and empty[0] == bam_sorted_file("@CO\tx\n", G["contigs"], b"", 1, window, host=True)[0]


def test_the_report_and_the_table_from_its_text(G, tmp_path):
    from bwamem_hip.lib import RECAL_APPLY_SUMMARY, bam_apply_recal, bam_recal
    from bwamem_hip.recal import read_recal_table, recal_apply_report_text, recal_table_text
    counted = bam_recal(G["stream"], G["contigs"], G["pac"], len(G["ref"]), host=True)
    path = tmp_path / "t.txt"
    path.write_text(recal_table_text(counted))
    a, ca = bam_apply_recal(G["stream"], str(path), host=True)                            # a path, the dict read from it and the counted dict itself: one table
    b, cb = bam_apply_recal(G["stream"], read_recal_table(str(path)), host=True)
    c, cc = bam_apply_recal(G["stream"], counted, host=True)
    assert a == b == c and a != G["stream"] and same_counts(ca, dict(summary=np.asarray(cb["summary"], np.int64), qual_hist=np.asarray(cc["qual_hist"], np.int64)))
    text = recal_apply_report_text(ca)
    rows = [ln.split("\t") for ln in text.splitlines()]
    assert [r[1] for r in rows if r[0] == "AS"] == list(RECAL_APPLY_SUMMARY) and [int(r[2]) for r in rows if r[0] == "AS"] == [int(v) for v in ca["summary"][:9]]
    aq = [(int(r[1]), int(r[2]), int(r[3])) for r in rows if r[0] == "AQ"]
    assert all(r[0] in ("AS", "AQ") for r in rows) and aq == [(q, int(ca["qual_hist"][0][q]), int(ca["qual_hist"][1][q])) for q in range(94) if ca["qual_hist"][0][q] or ca["qual_hist"][1][q]]
    assert sum(x[1] for x in aq) == sum(x[2] for x in aq) == ca["bases_seen"]


def test_the_appended_members_leave_older_records_valid():
    from bwamem_hip.lib import Recal, RecalOpt, SortedOpt, SortedResults, _sorted_file_api, load_library
    assert [f[0] for f in RecalOpt._fields_[-2:]] == ["apply", "no_count"] and [f[0] for f in Recal._fields_[-4:]] == ["apply_summary", "qual_hist", "apply_ms", "apply_windows"]
    L = _sorted_file_api(load_library())
    pac = np.zeros(16, np.uint8); lens = np.array([20, 12], np.int32)
    o = RecalOpt(6, 500, pac.ctypes.data, 32)                                             # positional, as before the members existed
    assert not o.apply and o.no_count == 0
    old = Recal.apply_summary.offset                                                      # the record's size before the members existed
    buf = (C.c_uint8 * C.sizeof(Recal))()
    C.memset(buf, 0xab, C.sizeof(Recal))
    C.memset(buf, 0, old)                                                                 # a zeroed record of the old size, canaries behind it
    rt = C.cast(buf, C.POINTER(Recal))
    rec = read("ACGT", 30)
    L.bmh_bam_recal_host.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(RecalOpt), C.POINTER(Recal)]
    L.bmh_recal_free.argtypes = [C.POINTER(Recal)]
    assert L.bmh_bam_recal_host(rec, len(rec), 2, lens.ctypes.data, C.byref(o), rt) == 0 and rt.contents.summary[0] == 1 and rt.contents.cycle_m
    assert bytes(buf[old:]) == b"\xab" * (C.sizeof(Recal) - old)
    L.bmh_recal_free(rt)
    assert bytes(buf[old:]) == b"\xab" * (C.sizeof(Recal) - old) and bytes(buf[:old]) == bytes(old)
    names = (C.c_char_p * 2)(b"c1", b"c2")
    so = SortedOpt(1, 0, 0, 14, 0, None, None, None, None, C.pointer(o))
    res = SortedResults(None, None, None)
    res.recal = rt
    bam, bai, nb, ni = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    assert L.bmh_bam_sorted_file_host(b"@CO\tx\n", 2, names, lens.ctypes.data, rec, len(rec), C.byref(so), C.byref(bam), C.byref(nb), C.byref(bai), C.byref(ni), C.byref(res)) == 0
    assert rt.contents.summary[0] == 1 and bytes(buf[old:]) == b"\xab" * (C.sizeof(Recal) - old)
    L.bmh_recal_free(rt)
    L.bmh_free.argtypes = [C.c_void_p]
    L.bmh_free(bam); L.bmh_free(bai)
    assert bytes(buf[old:]) == b"\xab" * (C.sizeof(Recal) - old)


def test_the_keywords_and_the_command_lines_refuse_what_does_not_go_together(capsys, tmp_path):
    from bwamem_hip import bam, mem
    from bwamem_hip.aligner import recal_request
    from bwamem_hip.lib import bam_sorted_file, recal_opt
    capsys.readouterr()
    for argv, msg in ((["--sort", "--apply-recal-report", "r.txt", "p", "r.fa"], "--apply-recal-report needs --apply-recal"), (["--apply-recal", "t.txt", "p", "r.fa"], "need --sort"),
                      (["--sort", "--apply-recal"], "option --apply-recal needs a value"), (["--sort", "--recal", "t.txt", "--apply-recal", "./t.txt", "p", "r.fa"], "name the same file")):
        assert mem.main(argv) == 2 and msg in capsys.readouterr().err, argv
    for argv, msg in ((["--apply-recal-report", "r.txt", "in.bam"], "--apply-recal-report needs --apply-recal"), (["--apply-recal"], "option --apply-recal needs a value"),
                      (["--recal", "t.txt", "--reference", "p", "--apply-recal", "t.txt", "in.bam"], "name the same file")):
        assert bam.main(argv) == 2 and msg in capsys.readouterr().err, argv
    no_table = tmp_path / "no_table.txt"
    no_table.write_text("XX\t1\n")
    out = tmp_path / "out.bam"
    assert bam.main(["--host", "--apply-recal", str(no_table), "-o", str(out), "in.bam"]) == 1 and "line 1 is no row" in capsys.readouterr().err and not out.exists()
    assert mem.main(["--sort", "--apply-recal", str(no_table), "-o", str(out), "p", "r.fa"]) == 1 and "line 1 is no row" in capsys.readouterr().err and not out.exists()
    with pytest.raises(ValueError, match="apply_recal_report needs apply_recal"):
        recal_request("align_files", True, apply_recal_report="r.txt")
    with pytest.raises(ValueError, match="apply_recal needs sort=True"):
        recal_request("align_files", False, apply_recal=hand_table(), sorted_out=False)
    with pytest.raises(ValueError, match="apply_recal_report needs apply_recal"):
        bam_sorted_file("@CO\tx\n", [("c1", 20)], b"", host=True, apply_recal_report="r.txt")
    with pytest.raises(ValueError, match="count=False needs apply"):
        recal_opt(count=False)
    req = recal_request("bam_post_file", True, apply_recal=hand_table())
    assert req["table"] is None and req["apply"]["max_cycle"] == 5


# ---------------------------------------------------------------------------------------------------------------- under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_requal_core_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_requal_core_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_requal_core.h", "bam_requal.h", "bam_recal_core.h", "bam_recal.h", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def run_core(tmp_path, cases):
    """cases: (table, window, stream) -> per case (status, index, code, tables, records, counts)"""
    fi, fo = str(tmp_path / "requal_case.bin"), str(tmp_path / "requal_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for t, window, s in cases:
            groups = [g for g in t["read_groups"] if t["read_groups"] != ["*"]]
            f.write(struct.pack("<iii", len(groups), t["min_qual"], t["max_cycle"]) + b"".join(g.encode() + b"\0" for g in groups))
            f.write(np.asarray(t["cycle_m"], dtype="<u8").tobytes() + np.asarray(t["context_m"], dtype="<u8").tobytes() + struct.pack("<IQ", window, len(s)) + s)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    res = np.fromfile(fo, dtype=np.uint8).tobytes()
    out, p = [], 0
    for t, _w, s in cases:
        rc, index, code = struct.unpack_from("<iQi", res, p); p += 16
        if rc != 0:
            out.append((rc, index, code, None, None, None))
            continue
        g, row = t["cycle_m"].shape[0], 17 + 2 * t["max_cycle"]
        tabs = np.frombuffer(res, dtype="<i2", count=g * 94 * row, offset=p).reshape(g, 94, row).copy(); p += 2 * tabs.size
        recs = res[p:p + len(s)]; p += len(s)
        w = np.frombuffer(res, dtype="<u8", count=16 + 188, offset=p).astype(np.int64); p += 8 * len(w)
        out.append((0, 0, 0, tabs, recs, dict(summary=w[:16], qual_hist=w[16:].reshape(2, 94))))
    assert p == len(res)
    return out


def test_core_under_sanitizers(tmp_path):
    contigs, ref, _pac, _hole = genome()
    ids = ["lane1", "lane2", "x"]
    t1, tg, hand = random_table(3), random_table(4, ids, max_cycle=33), hand_table()
    plain, grouped = synth_records(600, contigs, ref), synth_records(300, contigs, ref, seed=2, groups=ids)
    cases = [(t1, w, b"".join(plain)) for w in (0, 1, 7)] + [(tg, 25, b"".join(grouped)), (tg, 0, b""), (hand, 0, b"".join(rec for _w, rec, _q in HAND))]
    got = run_core(tmp_path, cases)
    for (t, _w, s), (rc, _i, _c, tabs, recs, counts) in zip(cases, got):
        want, wc = apply_model(s, t, tabs)
        assert rc == 0 and recs == b"".join(want) and same_counts(counts, wc) and np.abs(tabs - deltas(t)).max() <= 1
    assert np.array_equal(got[-1][3], deltas(hand)) and [quals(r) for r in split(got[-1][4])][:3] == [q for _w, _r, q in HAND[:3]]
    # about 1500 damaged streams: truncated records, tags that overrun, l_seq beyond the record, fields overwritten -- refused or equal to the model, and never a
    # byte outside the stream
    rng = np.random.default_rng(11)
    damaged = []
    for k in range(1500):
        recs = [bytearray(r) for r in grouped[(k % 8) * 5:(k % 8) * 5 + 5]]
        r = recs[int(rng.integers(0, 5))]
        l_name, n_ops, l_seq = r[12], struct.unpack_from("<H", r, 16)[0], struct.unpack_from("<I", r, 20)[0]
        kind = k % 5
        if kind == 0:                                                                     # the record cut short (the block_size follows)
            del r[-int(rng.integers(1, 40)):]
            struct.pack_into("<I", r, 0, len(r) - 4)
        elif kind == 1:                                                                   # tags cut short, or a tag's type or an array's count overwritten
            tags_at = 36 + l_name + 4 * n_ops + (l_seq + 1) // 2 + l_seq
            if rng.random() < 0.5:
                del r[-int(rng.integers(1, 12)):]
                struct.pack_into("<I", r, 0, len(r) - 4)
            else:
                r[int(rng.integers(tags_at, len(r)))] = int(rng.choice([0, ord("B"), ord("Z"), 0xff, ord("i")]))
        elif kind == 2:                                                                   # l_seq rewritten: a little, or far beyond the record
            struct.pack_into("<I", r, 20, int(rng.choice([max(0, l_seq + int(rng.integers(-3, 4))), l_seq + len(r), 0x7fffffff, 0xffffffff, 0])))
        elif kind == 3:                                                                   # bytes behind the fixed fields overwritten
            for at in rng.integers(36 + l_name, len(r), 3):
                r[int(at)] = int(rng.integers(0, 256))
        else:                                                                             # the name's length, the operations' count, the flag
            at = int(rng.choice([12, 16, 18, 19]))
            r[at] = int(rng.integers(0, 256))
        damaged.append(b"".join(bytes(x) for x in recs))
    got = run_core(tmp_path, [(tg, 2, s) for s in damaged])
    refused = rewritten = 0
    for s, (rc, index, code, tabs, recs, counts) in zip(damaged, got):
        try:
            from test_bam_sort import split_records
            whole = split_records(s)
        except (AssertionError, struct.error):
            assert rc == -2
            continue
        if any(len(x) < 36 + x[12] + 4 * struct.unpack_from("<H", x, 16)[0] for x in whole):  # (no whole record: the stream is refused before the step sees it)
            assert rc == -2
            continue
        want = apply_model(whole, tg, tabs if tabs is not None else None)
        if want[0] == "refused":
            refused += 1
            assert (rc, index, code) == (-2, want[1], want[2]), (want, rc, index, code)
        else:
            rewritten += 1
            assert rc == 0 and recs == b"".join(want[0]) and same_counts(counts, want[1])
    assert refused > 100 and rewritten > 100
