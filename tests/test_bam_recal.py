"""The recalibration table without a GPU: the Python model of tests/recal_model.py pinned by rows counted by hand; the host form against the model
on a table of cases -- one for every branch of the definition -- and on synthetic records; the windows of the host merge; the mask parser and its refusals by file
and line; the text and its inverse; the appended members of the sorted output's records; and csrc/bam_recal_core.h with the host form and the mask parser under
AddressSanitizer and UBSan (a stand-alone program, run as a child process)."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from recal_model import (ARRAYS, CAPPED, D, EQ, E_CUT, E_PLACEHOLDER, E_RG_ID, E_RG_NONE, E_RG_TYPE, E_SPAN, E_SUM, E_TAGS, F_FLAGS, F_MAPQ, F_NOOPS, F_NOQUAL, F_REF, H, I, KEPT, M, N, S,
                         SK_ANCHOR, SK_BASE, SK_MASK, SK_QUAL, WORDS, X, check_invariants, cut_record, equal, expect_rows, genome, hand_cases, mask_words, model, rrec, synth_records, table_cases,
                         SMALL_CONTIGS as CONTIGS, SMALL_LENS as LENS, SMALL_PAC as PAC, SMALL_REF as REF)

HERE = os.path.dirname(os.path.abspath(__file__))
# (the reference of the hand-counted cases, tests/recal_model.py: c1 = ACGT five times, c2 = GGGGCCCCAAAA)


def host(recs, mask=None, **kw):
    from bwamem_hip.lib import bam_recal
    return bam_recal(b"".join(recs), CONTIGS, PAC, len(REF), mask=None if mask is None else mask_words(mask), host=True, **kw)


def rows(r, keys=("CY", "CX")):
    from bwamem_hip.recal import recal_table_text
    return [ln for ln in recal_table_text(r).split("\n") if ln[:2] in keys]


def both(recs, mask=None, **kw):
    """the host form and the model over the same records: one table"""
    got = host(recs, mask, **kw)
    want = model(recs, LENS, REF, mask, groups=kw.get("read_groups"), min_qual=kw.get("min_qual", 6), max_cycle=kw.get("max_cycle", 500))
    assert equal(got, want), [k for k in ARRAYS if not np.array_equal(got[k], np.asarray(want[k], dtype=np.uint64))]
    check_invariants(got)
    return got


# ---------------------------------------------------------------------------------------------------------------- rows counted by hand

def test_a_forward_record_by_hand():
    # ACGA at c1:0 against ACGT: the fourth base is a mismatch.  Cycles 1 .. 4; contexts -, AC, CG, GA and -, -, ACG, CGA
    r = both([rrec(b"a", 0, 0, 0, 30, ((4, M),), "ACGA", 30)])
    assert rows(r) == ["CY\t*\t30\t1\tM\t1\t0", "CY\t*\t30\t2\tM\t1\t0", "CY\t*\t30\t3\tM\t1\t0", "CY\t*\t30\t4\tM\t1\t1",
                       "CY\t*\t45\t1\tI\t1\t0", "CY\t*\t45\t1\tD\t1\t0", "CY\t*\t45\t2\tI\t1\t0", "CY\t*\t45\t2\tD\t1\t0",
                       "CY\t*\t45\t3\tI\t1\t0", "CY\t*\t45\t3\tD\t1\t0", "CY\t*\t45\t4\tI\t1\t0", "CY\t*\t45\t4\tD\t1\t0",
                       "CX\t*\t30\t-\tM\t1\t0", "CX\t*\t30\tAC\tM\t1\t0", "CX\t*\t30\tCG\tM\t1\t0", "CX\t*\t30\tGA\tM\t1\t1",
                       "CX\t*\t45\t-\tI\t2\t0", "CX\t*\t45\t-\tD\t2\t0", "CX\t*\t45\tACG\tI\t1\t0", "CX\t*\t45\tACG\tD\t1\t0", "CX\t*\t45\tCGA\tI\t1\t0", "CX\t*\t45\tCGA\tD\t1\t0"]
    assert rows(r, ("RG", "QS")) == ["RG\t*\tM\t4\t1", "RG\t*\tI\t4\t0", "RG\t*\tD\t4\t0", "QS\t*\t30\tM\t4\t1", "QS\t*\t45\tI\t4\t0", "QS\t*\t45\tD\t4\t0"]


def test_a_reverse_second_read_by_hand():
    # ACT at c1:4 (ACG), 0x10 and the second of a pair: sequencing order is the reverse complement A G T, its first base the mismatch; cycles -1 .. -3
    r = both([rrec(b"b", 0, 4, 0x91, 30, ((3, M),), "ACT", 30)])
    assert rows(r) == ["CY\t*\t30\t-3\tM\t1\t0", "CY\t*\t30\t-2\tM\t1\t0", "CY\t*\t30\t-1\tM\t1\t1",
                       "CY\t*\t45\t-3\tI\t1\t0", "CY\t*\t45\t-3\tD\t1\t0", "CY\t*\t45\t-2\tI\t1\t0", "CY\t*\t45\t-2\tD\t1\t0", "CY\t*\t45\t-1\tI\t1\t0", "CY\t*\t45\t-1\tD\t1\t0",
                       "CX\t*\t30\t-\tM\t1\t1", "CX\t*\t30\tAG\tM\t1\t0", "CX\t*\t30\tGT\tM\t1\t0",
                       "CX\t*\t45\t-\tI\t2\t0", "CX\t*\t45\t-\tD\t2\t0", "CX\t*\t45\tAGT\tI\t1\t0", "CX\t*\t45\tAGT\tD\t1\t0"]
    # the first of a pair and a single read count their cycles upwards
    assert [ln.split("\t")[3] for ln in rows(both([rrec(b"b", 0, 4, 0x51, 30, ((3, M),), "ACG", 30)]), ("CY",))[:3]] == ["1", "2", "3"]
    assert [ln.split("\t")[3] for ln in rows(both([rrec(b"b", 0, 4, 0x90, 30, ((3, M),), "ACG", 30)]), ("CY",))[:3]] == ["1", "2", "3"]


def test_an_insertion_and_a_deletion_by_hand():
    # AC T G - A: 2M 1I 1M 1D 1M at c1:0.  Forward: the base before the I run (cycle 2) carries ins, the base before the D (cycle 4) del
    ops = ((2, M), (1, I), (1, M), (1, D), (1, M))
    r = both([rrec(b"c", 0, 0, 0, 30, ops, "ACTGA", 30)])
    errs = [ln for ln in rows(r) if ln.split("\t")[-1] != "0"]
    assert errs == ["CY\t*\t45\t2\tI\t1\t1", "CY\t*\t45\t4\tD\t1\t1", "CX\t*\t45\t-\tI\t2\t1", "CX\t*\t45\tCTG\tD\t1\t1"]
    # 0x10: the base behind the I run (stored 3: cycle 2) carries ins, the base behind the D (stored 4: cycle 1) del; sequencing order T C A G T
    r = both([rrec(b"c", 0, 0, 0x10, 30, ops, "ACTGA", 30)])
    errs = [ln for ln in rows(r) if ln.split("\t")[-1] != "0"]
    assert errs == ["CY\t*\t45\t1\tD\t1\t1", "CY\t*\t45\t2\tI\t1\t1", "CX\t*\t45\t-\tI\t2\t1", "CX\t*\t45\t-\tD\t2\t1"]


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_every_branch_by_hand(case):
    """one record for every branch of the definition: the rows of the text are the ones written out by hand in tests/recal_model.py"""
    _name, recs, mask, kw, obs = case
    assert rows(both(recs, mask, **kw)) == expect_rows(obs)


@pytest.mark.parametrize("case", table_cases(), ids=lambda c: c[0])
def test_the_table_of_cases_on_the_host(case):
    _name, recs, mask, kw = case
    both(recs, mask, **kw)


# ---------------------------------------------------------------------------------------------------------------- every branch, host form against model

def test_clips_and_events_at_the_ends():
    for flag in (0, 0x10):
        r = both([rrec(b"s", 0, 4, flag, 30, ((2, S), (3, M)), "TTACG", 30), rrec(b"t", 0, 4, flag, 30, ((3, M), (2, S)), "ACGTT", 30),
                  rrec(b"u", 0, 4, flag, 30, ((1, S), (3, M), (2, S)), "TACGTT", 30), rrec(b"h", 0, 4, flag, 30, ((5, H), (3, M), (2, H)), "ACG", 30),
                  rrec(b"hs", 0, 4, flag, 30, ((5, H), (1, S), (3, M), (1, S), (2, H)), "TACGT", 30)])
        assert int(r["summary"][KEPT]) == 15 and int(r["cycle_m"][..., 0].sum()) == 15 and r["cycle_m"][0, 30, 500 + 3:, 0].sum() == 0       # (cycles 1 .. 3 only: clips are not counted in)
        # I and D at the first and at the last kept base: the event whose base falls outside the kept bases is dropped
        first_i = both([rrec(b"i", 0, 4, flag, 30, ((1, S), (1, I), (3, M)), "TTACG", 30)])
        last_i = both([rrec(b"i", 0, 4, flag, 30, ((3, M), (1, I), (1, S)), "ACGTT", 30)])
        assert int(first_i["cycle_id"][..., 1].sum()) == (1 if flag else 0) and int(last_i["cycle_id"][..., 1].sum()) == (0 if flag else 1)
        first_d = both([rrec(b"d", 0, 4, flag, 30, ((1, D), (3, M)), "CGT", 30)])
        last_d = both([rrec(b"d", 0, 4, flag, 30, ((3, M), (1, D)), "ACG", 30)])
        assert int(first_d["cycle_id"][..., 2].sum()) == (1 if flag else 0) and int(last_d["cycle_id"][..., 2].sum()) == (0 if flag else 1)
        both([rrec(b"n", 0, 0, flag, 30, ((2, M), (3, N), (2, M)), "ACCG", 30), rrec(b"e", 0, 0, flag, 30, ((2, EQ), (2, X)), "ACTT", 30), rrec(b"one", 1, 0, flag, 30, ((1, M),), "G", 30),
              rrec(b"ii", 0, 0, flag, 30, ((2, M), (1, I), (1, I), (1, D), (1, I), (2, M)), "ACTTTGT", 30)])
    # = and X are not trusted: the bases decide
    r = both([rrec(b"e", 0, 0, 0, 30, ((2, EQ), (2, X)), "ATGT", 30)])
    assert [int(v) for v in r["cycle_m"][0, 30, 500:504, 1]] == [0, 1, 0, 0]


def test_bases_that_are_skipped():
    r = both([rrec(b"n", 0, 0, 0, 30, ((6, M),), "ACNTAC", 30)])                      # a base that is no ACGT: skipped, and the two contexts that reach over it are `none`
    assert int(r["summary"][SK_BASE]) == 1 and int(r["context_m"][0, 30, 16, 0]) == 2 and int(r["context_id"][0, 64, 0]) == 4
    r = both([rrec(b"q", 0, 0, 0, 30, ((3, M),), "ACG", [5, 6, 7])])
    assert int(r["summary"][SK_QUAL]) == 1 and int(r["cycle_m"][0, 6, 501, 0]) == 1 and int(r["cycle_m"][0, 7, 502, 0]) == 1
    assert int(both([rrec(b"q", 0, 0, 0, 30, ((3, M),), "ACG", [5, 6, 7])], min_qual=0)["summary"][SK_QUAL]) == 0
    assert int(both([rrec(b"q", 0, 0, 0, 30, ((3, M),), "ACG", [5, 6, 7])], min_qual=8)["summary"][SK_QUAL]) == 3
    both([rrec(b"q", 0, 0, 0, 30, ((3, M),), "ACG", [93, 94, 200])])                  # (qualities above 93 share 93)
    mask = np.zeros(32, bool); mask[5] = True
    r = both([rrec(b"m", 0, 4, 0, 30, ((4, M),), "ACGT", 30)], mask)                   # a masked M position
    assert int(r["summary"][SK_MASK]) == 1 and int(r["summary"][13]) == 1
    r = both([rrec(b"a", 0, 4, 0, 30, ((2, M), (2, I), (2, M)), "ACTTGT", 30), rrec(b"b", 0, 5, 0, 30, ((2, M), (2, I), (2, M)), "CGTTTA", 30)], mask)
    assert int(r["summary"][SK_ANCHOR]) == 2 and int(r["summary"][SK_MASK]) == 2      # (a: the anchor is position 5; b: position 5 is its own first base)
    both([rrec(b"i0", 0, 0, 0, 30, ((2, I), (2, M)), "TTAC", 30)], np.ones(32, bool))   # (an insertion in front of the contig's first base has no anchor)
    hole = np.zeros(32, bool); hole[20:24] = True                                    # a hole of the reference (.amb): c2's G's
    r = both([rrec(b"h", 1, 2, 0, 30, ((4, M),), "GGCC", 30)], hole)
    assert int(r["summary"][SK_MASK]) == 2


@pytest.mark.parametrize("cap", (1, 2, 500))
def test_cycles_around_the_cap(cap):
    for n in (cap - 1, cap, cap + 1):
        if n < 1:
            continue
        ref = np.resize(REF[:20], n)
        recs = [rrec(b"f", 0, 0, fl, 30, ((min(n, 20), M),) if n <= 20 else ((20, M), (n - 20, I)), "".join("ACGT"[c] for c in ref), 30) for fl in (0, 0x91, 0x10)]
        r = both(recs, max_cycle=cap)
        assert int(r["summary"][CAPPED]) == 3 * max(0, n - cap)


def test_every_filter_reason_and_every_refusal():
    ok = rrec(b"ok", 0, 0, 0, 30, ((4, M),), "ACGT", 30)
    left = [rrec(b"r1", -1, 0, 0, 30), rrec(b"r2", 2, 0, 0, 30), rrec(b"f4", 0, 0, 0x4, 30), rrec(b"f100", 0, 0, 0x100, 30), rrec(b"f200", 0, 0, 0x200, 30), rrec(b"f400", 0, 0, 0x400, 30),
            rrec(b"q0", 0, 0, 0, 0), rrec(b"q255", 0, 0, 0, 255), rrec(b"nq", 0, 0, 0, 30, qual=None), rrec(b"l0", 0, 0, 0, 30, ((3, N),), "", 30), rrec(b"no", 0, 0, 0, 30, (), "ACGT", 30),
            rrec(b"sup", 0, 0, 0x800, 30, ((4, M),), "ACGT", 30)]
    r = both([ok] + left)
    assert [int(r["summary"][k]) for k in (F_REF, F_FLAGS, F_MAPQ, F_NOQUAL, F_NOOPS)] == [2, 4, 2, 2, 1] and int(r["summary"][1]) == 2
    # a record that is left out is not read further: its operations may be anything
    both([rrec(b"f", 0, 0, 0x4, 30, ((9, M),), "ACGT", 30, b"XYZ")])
    from bwamem_hip.lib import bam_recal
    cases = ((E_SUM, rrec(b"x", 0, 0, 0, 30, ((5, M),), "ACGT", 30), None), (E_SUM, rrec(b"x", 0, 0, 0, 30, ((3, M),), "ACGT", 30), None),
             (E_PLACEHOLDER, rrec(b"x", 0, 0, 0, 30, ((4, S), (9, N)), "ACGT", 30, b"CGBI\1\0\0\0\x40\0\0\0"), None),
             (E_SPAN, rrec(b"x", 0, 17, 0, 30, ((4, M),), "ACGT", 30), None), (E_SPAN, rrec(b"x", 0, -1, 0, 30, ((4, M),), "ACGT", 30), None),
             (E_SPAN, rrec(b"x", 1, 9, 0, 30, ((2, M), (2, D), (2, M)), "ACGT", 30), None), (E_TAGS, rrec(b"x", 0, 0, 0, 30, ((4, M),), "ACGT", 30, b"NMC"), None),
             (E_TAGS, rrec(b"x", 0, 0, 0, 30, ((4, M),), "ACGT", 30, b"XYZab"), None), (E_RG_NONE, ok, ["a"]),
             (E_RG_TYPE, rrec(b"x", 0, 0, 0, 30, ((4, M),), "ACGT", 30, b"RGA!"), ["a"]), (E_RG_ID, rrec(b"x", 0, 0, 0, 30, ((4, M),), "ACGT", 30, b"RGZab\0"), ["a", "abc"]),
             (E_CUT, cut_record(), None))
    for code, rec, groups in cases:
        recs = [ok if groups is None else rrec(b"g", 0, 0, 0, 30, ((4, M),), "ACGT", 30, b"RGZa\0"), rrec(b"f", 0, 0, 0x4, 30), rec, rec]
        assert model(recs, LENS, REF, None, groups=groups) == ("refused", 2, code)
        with pytest.raises(ValueError) as e:
            bam_recal(b"".join(recs), CONTIGS, PAC, len(REF), read_groups=groups, host=True)
        assert str(e.value) == "bmh_bam_recal: bmh_bam_recal_host: record 2 " + WORDS[code]
    # a span that ends exactly at the contig's end is taken; groups: the ID decides, whatever else the record carries
    both([rrec(b"x", 0, 16, 0, 30, ((4, M),), "ACGT", 30), rrec(b"y", 1, 8, 0, 30, ((2, M), (2, D)), "AA", 30)])
    r = both([rrec(b"g", 0, 0, 0, 30, ((4, M),), "ACGT", 30, b"NMC\0RGZabc\0"), rrec(b"h", 0, 0, 0, 30, ((4, M),), "ACGT", 30, b"RGZa\0RGZabc\0")], read_groups=["a", "abc"])
    assert [int(v) for v in r["cycle_id"][:, :, 0].sum(axis=1)] == [4, 4]


def test_the_options_are_checked():
    from bwamem_hip.lib import bam_recal, bam_sorted_file
    ok = rrec(b"ok", 0, 0, 0, 30, ((4, M),), "ACGT", 30)
    for kw, words in ((dict(min_qual=94), "recal_min_qual"), (dict(min_qual=-1), "recal_min_qual"), (dict(max_cycle=0), "recal_max_cycle"), (dict(max_cycle=65536), "recal_max_cycle"),
                      (dict(read_groups=["g%d" % k for k in range(256)]), "at most 255"), (dict(read_groups=["a", "a"]), "twice"), (dict(max_cycle=65535, read_groups=["a%d" % k for k in range(200)]), "2\\^28")):
        with pytest.raises(ValueError, match=words):
            bam_recal(ok, CONTIGS, PAC, len(REF), host=True, **kw)
    with pytest.raises(ValueError, match="lies outside the reference"):
        bam_recal(ok, CONTIGS, PAC, 30, host=True)
    with pytest.raises(ValueError, match="a mask of 2 words"):
        bam_recal(ok, CONTIGS, PAC, len(REF), mask=np.zeros(2, np.uint64), host=True)
    with pytest.raises(ValueError, match="needs the reference"):
        bam_sorted_file("@CO\tx\n", CONTIGS, ok, host=True, recal=dict(l_pac=len(REF)))
    assert both([ok, ok], max_cycle=65535)["cycle_m"].shape == (1, 94, 131070, 2)


# ---------------------------------------------------------------------------------------------------------------- synthetic records, windows

@pytest.fixture(scope="module")
def G():
    contigs, ref, pac, hole = genome()
    mask = np.zeros(len(ref), bool); mask[hole[0]:hole[0] + hole[1]] = True; mask[::53] = True
    recs = synth_records(3000, contigs, ref)
    return dict(contigs=contigs, lens=[c[1] for c in contigs], ref=ref, pac=pac, mask=mask, words=mask_words(mask), recs=recs, want=model(recs, [c[1] for c in contigs], ref, mask))


def test_the_host_form_on_synthetic_records(G):
    from bwamem_hip.lib import bam_recal
    got = bam_recal(b"".join(G["recs"]), G["contigs"], G["pac"], len(G["ref"]), mask=G["words"], host=True)
    assert equal(got, G["want"])
    check_invariants(got)
    s = got["summary"]
    assert s[1] > 2500 and got["cycle_m"][..., 1].sum() > 100 and got["cycle_id"][..., 1].sum() > 100 and got["cycle_id"][..., 2].sum() > 100 and all(s[k] > 0 for k in (SK_BASE, SK_QUAL, SK_MASK, SK_ANCHOR))
    ids = ["lane1", "lane2", "x"]
    recs = synth_records(400, G["contigs"], G["ref"], seed=2, groups=ids)
    got = bam_recal(b"".join(recs), G["contigs"], G["pac"], len(G["ref"]), mask=G["words"], host=True, read_groups=ids, max_cycle=60)
    assert equal(got, model(recs, G["lens"], G["ref"], G["mask"], groups=ids, max_cycle=60)) and got["read_groups"] == ids


@pytest.mark.parametrize("window", (0, 1, 7, 25))
def test_the_windows_of_the_host_merge(G, window, tmp_path):
    from test_bam_sort import BamFile
    from bwamem_hip.lib import bam_post, bam_sorted_file
    recs = [r[:18] + bytes([r[18] & 0x14, r[19] & 0x6]) + r[20:] for r in G["recs"][:80] if r[7] < 0x80]  # (single primary reads on a contig: marking takes every name as one template)
    recs += [r[:36] + b"z" + r[37:] for r in recs[:6]]                                  # (duplicates under other names)
    s = b"".join(recs)
    kw = dict(pac=G["pac"], l_pac=len(G["ref"]), mask=G["words"])
    for markdup in (False, True):
        plain = bam_sorted_file("@CO\tx\n", G["contigs"], s, 1, window, host=True, markdup=markdup)
        got = bam_sorted_file("@CO\tx\n", G["contigs"], s, 1, window, host=True, markdup=markdup, recal=kw)
        assert got[:-1] == plain
        assert equal(got[-1], model(BamFile(got[0]).stream, G["lens"], G["ref"], G["mask"]))
        check_invariants(got[-1])
    assert any(r[19] & 0x4 for r in BamFile(got[0]).recs)
    # the stand-alone post-processing of a file takes the same record
    src = tmp_path / "in.bam"
    src.write_bytes(bam_sorted_file("@HD\tVN:1.6\tSO:unsorted\n", G["contigs"], s, 1, 0, host=True)[0])
    out = []
    r = bam_post(str(src), out.append, host=True, window=window, markdup=True, recal=kw)
    assert equal(r["recal"], model(BamFile(b"".join(out)).stream, G["lens"], G["ref"], G["mask"])) and BamFile(b"".join(out)).stream == BamFile(got[0]).stream
    assert bam_sorted_file("@CO\tx\n", G["contigs"], b"", 1, window, host=True, recal=kw)[-1]["summary"][0] == 0


# ---------------------------------------------------------------------------------------------------------------- the mask

VCF = "##fileformat=VCFv4.2\n##contig=<ID=c1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n\nc1\t3\t.\tG\tA\t.\t.\t.\nc2\t11\trs1\tAA\tA\t.\t.\t.\nc1\t20\t.\tT\tC\t.\t.\t.\n"
BED = "track name=x\nbrowser position c1:1-5\n# a comment\n\nc1\t4\t8\tname\nc2 0 2\nc1\t19\t20\n"


def bits(m, n=32):
    return [i for i in range(n) if int(m[i >> 6]) >> (i & 63) & 1]


def test_the_mask_parser(tmp_path):
    from bwamem_hip.lib import known_sites_mask
    v, b = tmp_path / "k.vcf", tmp_path / "k.bed"
    v.write_text(VCF); b.write_text(BED)
    vz, bz = tmp_path / "k.vcf.gz", tmp_path / "k.bed.gz"
    vz.write_bytes(gzip.compress(VCF.encode())); bz.write_bytes(gzip.compress(BED.encode()))
    want_v, want_b = [2, 19, 30, 31], [4, 5, 6, 7, 19, 20, 21]
    for pv, pb in ((v, b), (vz, bz)):
        assert bits(known_sites_mask([str(pv)], CONTIGS)) == want_v and bits(known_sites_mask(str(pb), CONTIGS)) == want_b
        assert bits(known_sites_mask([str(pb), str(pv), str(pb)], CONTIGS)) == sorted(set(want_v + want_b))            # (order does not matter, overlaps are fine)
    assert bits(known_sites_mask([], CONTIGS, holes=[(18, 4), (31, 1)])) == [18, 19, 20, 21, 31] and known_sites_mask([], CONTIGS).shape == (1,)
    (tmp_path / "last.bed").write_text("c1\t0\t1")                                       # (a last line without its newline)
    assert bits(known_sites_mask([str(tmp_path / "last.bed")], CONTIGS)) == [0]
    refused = (("c3\t1\t2\n", "bed", 1, "contig c3 is not among"), ("c1\t1\t2\nc1\t19\t21\n", "bed", 2, "lies outside contig c1"), ("c1\t5\t4\n", "bed", 1, "lies outside"),
               ("\nc1\t1\n", "bed", 2, "2 fields where a BED line has at least 3"), ("c1\tx\t2\n", "bed", 1, "start x is no number"), ("c1\t1\t2.5\n", "bed", 1, "end 2.5 is no number"),
               ("#CHROM\tPOS\nc1\t0\t.\tA\n", "vcf", 2, "lies outside contig"), ("#CHROM\nc1\t20\t.\tAC\tA\n", "vcf", 2, "lies outside contig c1"), ("##fileformat=VCFv4.2\nc1\t2\t.\n", "vcf", 2, "3 fields where a VCF line"),
               ("##fileformat=VCFv4.2\nc9\t2\t.\tA\n", "vcf", 2, "contig c9"), ("##fileformat=VCFv4.2\n\nc1\t-2\t.\tA\n", "vcf", 3, "POS -2 is no number"))
    for k, (text, ext, line, words) in enumerate(refused):
        p = tmp_path / ("bad%d.%s" % (k, ext))
        p.write_text(text)
        with pytest.raises(ValueError) as e:
            known_sites_mask([str(b), str(p)], CONTIGS)
        assert "%s line %d: " % (p, line) in str(e.value) and words in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        known_sites_mask([str(tmp_path / "none.vcf")], CONTIGS)


# ---------------------------------------------------------------------------------------------------------------- the text, the records

def test_the_text_and_its_inverse(G, tmp_path):
    from bwamem_hip.lib import bam_recal
    from bwamem_hip.recal import read_recal_table, recal_empirical_quality, recal_event_tables, recal_table_text, write_recal_table
    ids = ["b", "a"]
    recs = synth_records(300, G["contigs"], G["ref"], seed=4, groups=ids)
    r = bam_recal(b"".join(recs), G["contigs"], G["pac"], len(G["ref"]), mask=G["words"], host=True, read_groups=ids, max_cycle=90)
    r["known_sites"] = ["a.vcf", "b.bed"]
    text = recal_table_text(r)
    write_recal_table(r, str(tmp_path / "t.txt"))
    back = read_recal_table(str(tmp_path / "t.txt"))
    assert equal(back, r) and back["read_groups"] == ids and back["known_sites"] == r["known_sites"] and (back["min_qual"], back["max_cycle"]) == (6, 90)
    assert recal_table_text(back) == text
    lines = text.split("\n")
    assert lines[:7] == ["AR\tmin_qual\t6", "AR\tmax_cycle\t90", "AR\tindel_quality\t45", "AR\tmismatch_context\t2", "AR\tindel_context\t3", "AR\tread_group\tb", "AR\tread_group\ta"]
    assert "AR\tknown_sites\ta.vcf" in lines and "AR\tmasked_positions\t%d" % int(G["mask"].sum()) in lines and "SN\trecords_seen\t300" in lines
    cy = [ln.split("\t") for ln in lines if ln.startswith("CY")]
    assert all(int(f[5]) > 0 for f in cy)                                                           # (no row without an observation)
    order = [(ids.index(f[1]), int(f[2]), int(f[3]), "MID".index(f[4])) for f in cy]
    assert order == sorted(order) and any(c < 0 for _g, _q, c, _e in order)
    cx = [ln.split("\t") for ln in lines if ln.startswith("CX")]
    order = [(ids.index(f[1]), int(f[2]), f[3], "MID".index(f[4])) for f in cx]
    assert order == sorted(order) and any(f[3] == "-" for f in cx)
    t = recal_event_tables(r)
    assert int(t["group"][:, 1, 0].sum()) == int(t["group"][:, 2, 0].sum()) == int(r["cycle_id"][..., 0].sum())
    broken = [ln for ln in lines if ln]
    k = next(i for i, ln in enumerate(broken) if ln.startswith("QS"))
    broken[k] = broken[k].rsplit("\t", 2)[0] + "\t1\t0"
    with pytest.raises(ValueError, match="line %d: the row is not the sum" % (k + 1)):
        read_recal_table(broken)
    with pytest.raises(ValueError, match="line 1 is no row"):
        read_recal_table(["XX\t1"])
    assert recal_empirical_quality(0, 0) == 3 and recal_empirical_quality(998, 0) == 30 and recal_empirical_quality(98, 9) == 10
    assert list(recal_empirical_quality([998, 98], [0, 9])) == [30, 10]


def test_the_appended_members_leave_positional_records_valid():
    import ctypes as C
    from bwamem_hip.lib import BamStats, BamStatsOpt, Coverage, CoverageOpt, MarkdupCounts, MarkdupOpt, SortedOpt, SortedResults, _sorted_file_api, load_library, SORTED_PARTS
    o = SortedOpt(1, 0, 0, 14, 0, None, None, None, None)
    assert not o.recal and SortedOpt._fields_[-1][0] == "recal" and [f[0] for f in SortedResults._fields_[-3:]] == ["recal", "recal_ms", "recal_windows"] and SORTED_PARTS["recal"] == 64
    res = SortedResults(None, None, None)
    assert not res.recal
    L = _sorted_file_api(load_library())
    d = SortedOpt()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    L.bmh_sorted_opt_default(C.byref(d))
    assert not d.recal and not d.stats and d.level == 1
    assert all(issubclass(t, C.Structure) for t in (MarkdupOpt, MarkdupCounts, CoverageOpt, Coverage, BamStatsOpt, BamStats))


_FAILED_CALL = r"""
import ctypes as C, sys
from bwamem_hip.lib import Recal, RecalOpt, SortedOpt, SortedResults, load_library
import numpy as np
L = load_library()
rec = bytes.fromhex(sys.argv[1])
pac = np.zeros(16, np.uint8); lens = np.array([20, 12], np.int32)
o = RecalOpt(6, 500, pac.ctypes.data, 32)
rt = Recal()
C.memset(C.byref(rt), 0xff, C.sizeof(rt))
L.bmh_bam_recal_host.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(RecalOpt), C.POINTER(Recal)]
assert L.bmh_bam_recal_host(rec, len(rec), 2, lens.ctypes.data, C.byref(o), C.byref(rt)) == -2
assert not rt.cycle_m and not rt.cycle_id and not rt.context_m and not rt.context_id
L.bmh_recal_free.argtypes = [C.POINTER(Recal)]
L.bmh_recal_free(C.byref(rt))
C.memset(C.byref(rt), 0xff, C.sizeof(rt))
names = (C.c_char_p * 2)(b"c1", b"c2")
so = SortedOpt(1, 0, 0, 14, 0, None, None, None, None, C.pointer(o))
res = SortedResults(None, None, None)
res.recal = C.pointer(rt)
bam, bai, nb, ni = C.c_void_p(1), C.c_void_p(1), C.c_uint64(), C.c_uint64()
L.bmh_bam_sorted_file_host.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(SortedOpt), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(SortedResults)]
assert L.bmh_bam_sorted_file_host(b"@CO\tx\n", 2, names, lens.ctypes.data, rec, len(rec), C.byref(so), C.byref(bam), C.byref(nb), C.byref(bai), C.byref(ni), C.byref(res)) == -2
assert not bam.value and not bai.value and not rt.cycle_m and not rt.cycle_id and not rt.context_m and not rt.context_id
L.bmh_recal_free(C.byref(rt))
res.recal = None                                                   # the record is required exactly when the option is set
assert L.bmh_bam_sorted_file_host(b"@CO\tx\n", 2, names, lens.ctypes.data, b"", 0, C.byref(so), C.byref(bam), C.byref(nb), C.byref(bai), C.byref(ni), C.byref(res)) == -2
print("ok")
"""


def test_a_failed_call_leaves_every_array_null():
    import sys
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(HERE, "..", "bwa-mem_gpu_amd")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    bad = rrec(b"x", 0, 17, 0, 30, ((4, M),), "ACGT", 30)
    r = subprocess.run([sys.executable, "-c", _FAILED_CALL, bad.hex()], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stdout.decode().strip() == "ok", r.stderr.decode(errors="replace")[-2000:]


def test_the_command_lines_refuse_what_does_not_go_together(capsys):
    from bwamem_hip import bam, mem
    capsys.readouterr()
    for argv, msg in ((["--recal", "t.txt", "p", "r.fa"], "need --sort"), (["--sort", "--known-sites", "k.vcf", "p", "r.fa"], "need --recal"), (["--sort", "--recal-min-qual", "5", "p", "r.fa"], "need --recal"),
                      (["--sort", "--recal-max-cycle", "0", "--recal", "t", "p", "r.fa"], "option --recal-max-cycle needs a whole number, 1 .. 65535"), (["--sort", "--recal"], "option --recal needs a value")):
        assert mem.main(argv) == 2 and msg in capsys.readouterr().err, argv
    for argv, msg in ((["--recal", "t.txt", "in.bam"], "--recal needs --reference"), (["--reference", "p", "in.bam"], "--reference needs --recal"), (["--known-sites", "k.vcf", "in.bam"], "need --recal"),
                      (["--recal-min-qual", "94", "--recal", "t", "--reference", "p", "in.bam"], "option --recal-min-qual needs a quality, 0 .. 93")):
        assert bam.main(argv) == 2 and msg in capsys.readouterr().err, argv


# ---------------------------------------------------------------------------------------------------------------- under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_recal_core_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_recal_core_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_recal_core.h", "bam_recal.h", "bam_recal_host.cpp", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def run_core(tmp_path, cases):
    """cases: ("table", lens, pac, l_pac, mask words or None, groups, min_qual, max_cycle, window, stream) or ("mask", contigs, file name, piece, text)"""
    fi, fo = str(tmp_path / "recal_case.bin"), str(tmp_path / "recal_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            if c[0] == "mask":
                _k, contigs, name, piece, text = c
                f.write(struct.pack("<II", 1, len(contigs)) + b"".join(struct.pack("<i", ln) + nm.encode() + b"\0" for nm, ln in contigs))
                f.write(struct.pack("<I", piece) + name.encode() + b"\0" + struct.pack("<Q", len(text)) + text)
                continue
            _k, lens, pac, l_pac, words, groups, min_qual, max_cycle, window, s = c
            f.write(struct.pack("<II", 0, len(lens)) + struct.pack("<%di" % len(lens), *lens) + struct.pack("<iiIII", min_qual, max_cycle, window, 0 if words is None else 1, len(groups or [])))
            f.write(b"".join(g.encode() + b"\0" for g in groups or []) + struct.pack("<Q", l_pac) + bytes(pac[:(l_pac + 3) // 4]))
            if words is not None:
                f.write(np.asarray(words, dtype="<u8").tobytes())
            f.write(struct.pack("<Q", len(s)) + s)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:verify_asan_link_order=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    res = np.fromfile(fo, dtype=np.uint8).tobytes()
    out, p = [], 0
    for c in cases:
        if c[0] == "mask":
            rc = struct.unpack_from("<i", res, p)[0]; msg = res[p + 4:p + 260].split(b"\0")[0].decode(); p += 260
            words = None
            if rc == 0:
                n = (sum(ln for _nm, ln in c[1]) + 63) // 64
                words = np.frombuffer(res, dtype="<u8", count=n, offset=p).copy(); p += 8 * n
            out.append((rc, msg, words))
            continue
        rc, index, code = struct.unpack_from("<iQi", res, p); p += 16
        if rc != 0:
            out.append((rc, index, code, None))
            continue
        g, cy = max(len(c[5] or []), 1), 2 * c[7]
        sizes = (16, g * 94 * cy * 2, g * cy * 3, g * 94 * 17 * 2, g * 65 * 3)
        w = np.frombuffer(res, dtype="<u8", count=sum(sizes), offset=p).copy(); p += 8 * len(w)
        parts = np.split(w, np.cumsum(sizes)[:-1])
        out.append((0, 0, 0, dict(summary=parts[0], cycle_m=parts[1].reshape(g, 94, cy, 2), cycle_id=parts[2].reshape(g, cy, 3), context_m=parts[3].reshape(g, 94, 17, 2),
                                  context_id=parts[4].reshape(g, 65, 3))))
    assert p == len(res)
    return out


def test_core_under_sanitizers(G, tmp_path):
    lens, pac, n = G["lens"], G["pac"], len(G["ref"])
    cases = [("table", lens, pac, n, G["words"], None, 6, 500, w, b"".join(G["recs"])) for w in (0, 1, 7)]
    ids = ["lane1", "lane2", "x"]
    grouped = synth_records(300, G["contigs"], G["ref"], seed=2, groups=ids)
    cases.append(("table", lens, pac, n, None, ids, 0, 33, 25, b"".join(grouped)))
    got = run_core(tmp_path, cases)
    for rc, _i, _c, r in got[:3]:
        assert rc == 0 and equal(r, G["want"])
    assert got[3][0] == 0 and equal(got[3][3], model(grouped, lens, G["ref"], None, groups=ids, min_qual=0, max_cycle=33))
    # a reference and a mask of exactly the contigs' size, records that touch their last base
    small = [rrec(b"e", 0, 16, 0, 30, ((4, M),), "ACGT", 30), rrec(b"f", 1, 8, 0x10, 30, ((2, M), (2, I), (2, M), (1, S)), "AATTAAC", 30), rrec(b"g", 1, 11, 0, 30, ((1, M), (3, I)), "ATTT", 30)]
    mask = np.zeros(32, bool); mask[31] = True
    (rc, _i, _c, r), = run_core(tmp_path, [("table", LENS, PAC, 32, mask_words(mask), None, 6, 2, 0, b"".join(small))])
    assert rc == 0 and equal(r, model(small, LENS, REF, mask, max_cycle=2))
    # the mask parser, the text in pieces of every small size
    masks = run_core(tmp_path, [("mask", CONTIGS, "k", piece, text.encode()) for text in (VCF, BED) for piece in (0, 1, 2, 3, 5, 64)] +
                     [("mask", CONTIGS, "bad.bed", 1, b"c1\t1\t2\nc1\t19\t21"), ("mask", CONTIGS, "bad.vcf", 4, b"#CHROM\nc1\t21\t.\tA\n"), ("mask", CONTIGS, "cut.vcf", 0, b"#CHROM\nc1\t2")])
    assert all(rc == 0 and bits(w) == ([2, 19, 30, 31] if k < 6 else [4, 5, 6, 7, 19, 20, 21]) for k, (rc, _m, w) in enumerate(masks[:12]))
    assert [(rc, "line %d" % ln in msg) for (rc, msg, _w), ln in zip(masks[12:], (2, 2, 2))] == [(-2, True)] * 3
    # about 1500 damaged streams: bytes of a synthetic stream overwritten, operation lengths off by one, tags and records cut short -- refused or counted,
    # never out of bounds, and whatever the host form says the model says too
    rng = np.random.default_rng(11)
    base = G["recs"][:40]
    damaged = []
    for k in range(1500):
        recs = [bytearray(r) for r in base[(k % 8) * 5:(k % 8) * 5 + 5]]
        r = recs[int(rng.integers(0, 5))]
        l_name, n_ops, l_seq = r[12], struct.unpack_from("<H", r, 16)[0], struct.unpack_from("<I", r, 20)[0]
        kind = k % 5
        if kind == 0 and n_ops:                                                                       # an operation's length off by one, or another operation
            at = 36 + l_name + 4 * int(rng.integers(0, n_ops))
            v = struct.unpack_from("<I", r, at)[0]
            struct.pack_into("<I", r, at, max(0, v + (16 if rng.random() < 0.5 else -16)) if rng.random() < 0.7 else (v & ~15) | int(rng.integers(0, 16)))
        elif kind == 1:                                                                               # tags cut short (the block_size follows)
            cut = int(rng.integers(1, 12))
            del r[-cut:]
            struct.pack_into("<I", r, 0, len(r) - 4)
        elif kind == 2:                                                                               # l_seq or pos rewritten
            if rng.random() < 0.5:
                struct.pack_into("<I", r, 20, max(0, l_seq + int(rng.integers(-3, 4))))
            else:
                struct.pack_into("<i", r, 8, int(rng.choice([-1, 2590, 2599, 1699, 1 << 30])))
        elif kind == 3:                                                                               # bytes behind the fixed fields overwritten
            for at in rng.integers(36 + l_name, len(r), 3):
                r[int(at)] = int(rng.integers(0, 256))
        else:                                                                                         # the fixed fields' flag, mapq, refID
            r[int(rng.choice([4, 13, 18, 19]))] = int(rng.integers(0, 256))
        damaged.append(b"".join(bytes(x) for x in recs))
    got = run_core(tmp_path, [("table", lens, pac, n, G["words"], None, 6, 500, 2, s) for s in damaged])
    refused = 0
    for s, (rc, index, code, r) in zip(damaged, got):
        try:
            from test_bam_sort import split_records
            recs = split_records(s)
        except (AssertionError, struct.error):
            assert rc == -2
            continue
        if any(len(x) < 36 + x[12] + 4 * struct.unpack_from("<H", x, 16)[0] for x in recs):           # (no whole record: the stream is refused before the table sees it)
            assert rc == -2
            continue
        want = model(recs, lens, G["ref"], G["mask"])
        if isinstance(want, tuple):
            refused += 1
            assert (rc, index, code) == (-2, want[1], want[2]), (want, rc, index, code)
        else:
            assert rc == 0 and equal(r, want)
    assert 100 < refused < 1400
