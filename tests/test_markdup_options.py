"""The options of duplicate marking as one record (bmh_markdup_opt_t): every valid combination of read groups, an optical distance, a barcode tag
and barcode edits over one small stream, on the host.  What the combinations must agree on is written in the rules, not measured: the optical step only counts,
so a call's records and its eight counts are those of the same call without the distance; the templates without a barcode are a property of the stream and the
tag alone.  Every invalid combination raises the ValueError the keywords have always raised.  The same stream and combinations run on the device in
test_markdup_options_gpu.py."""
import ctypes as C
import itertools

import pytest

from bwamem_hip.lib import (BARCODE_GROUP_COUNTS, MARKDUP_COUNTS, OPTICAL_COUNTS, MarkdupCounts, MarkdupOpt, SortedOpt, SortedResults, _markdup_api, _sorted_file_api, bam_markdup,
                            bam_sorted_file, load_library)
from test_bam_dup import CONTIGS
from test_bam_umi import GROUPS, render
from test_bam_umi_edits import reads

HDR = "@HD\tVN:1.6\n"
DISTANCE = 25


def option_stream() -> bytes:
    """60 templates of test_bam_umi_edits.reads on three positions -- three read groups of two libraries, two tiles, barcodes a mismatch or two apart -- where
    of the pairs of a position every third is a copy of an earlier one a few pixels away: duplicates that are optical ones too"""
    rs, seen = reads(n=60, seed=3, n_pos=3), {}
    for d in rs:
        if d["kind"] != "pair":
            continue
        earlier = seen.setdefault(d["pos"], [])
        if len(earlier) % 3 == 2:
            src = earlier[len(earlier) // 3]
            d.update(umi=src["umi"], rg=src["rg"], swap=src["swap"], loc=(src["loc"][0], src["loc"][1] + 3, src["loc"][2] + 2))
        elif len(earlier) % 3 == 1 and earlier[-1]["umi"] is not None:      # ... and every third other the pair before it under a barcode one mismatch away
            src = earlier[-1]
            d.update(umi=src["umi"][:-1] + (b"A" if src["umi"][-1:] != b"A" else b"C"), rg=src["rg"], swap=src["swap"])
        earlier.append(d)
    return render(rs, "tag", True)


def combinations():
    """every valid combination of the four options, as keywords: edits need the tag"""
    out = []
    for groups, optical, tag, edits in itertools.product((False, True), (False, True), (False, True), (False, True)):
        if edits and not tag:
            continue
        kw = {}
        if groups:
            kw["read_groups"] = GROUPS
        if optical:
            kw["optical_distance"] = DISTANCE
        if tag:
            kw["barcode_tag"] = "RX"
        if edits:
            kw["barcode_edits"] = 1
        out.append(kw)
    return out


COMBOS = combinations()
_STREAM, _HOST = [], {}


def stream() -> bytes:
    if not _STREAM:
        _STREAM.append(option_stream())
    return _STREAM[0]


def kw_id(kw: dict) -> str:
    return "+".join(k for k in kw) or "plain"


def host_markdup(kw: dict):
    """bam_markdup(host=True) under kw, computed once and shared"""
    key = kw_id(kw)
    if key not in _HOST:
        _HOST[key] = bam_markdup(stream(), host=True, **kw)
    return _HOST[key]


def without(kw: dict, *names) -> dict:
    return {k: v for k, v in kw.items() if k not in names}


def test_the_stream_exercises_every_option():
    c = host_markdup(dict(read_groups=GROUPS, optical_distance=DISTANCE, barcode_tag="RX", barcode_edits=1))[1]
    assert c["templates"] == 60 and len(c["libraries"]) == 2
    assert c["duplicate_pairs"] > 0 and c["duplicate_fragments"] > 0 and c["optical_duplicate_pairs"] > 0 and c["templates_without_barcode"] > 0
    assert c["pair_barcodes_inferred"] < c["pair_barcodes_observed"]      # (barcodes were joined)
    exact = host_markdup(dict(read_groups=GROUPS, barcode_tag="RX"))[1]
    assert exact["duplicate_pairs"] < c["duplicate_pairs"] < host_markdup(dict(read_groups=GROUPS))[1]["duplicate_pairs"]      # (every option changes the answer)


def test_default_record():
    L = _markdup_api(load_library())
    o = MarkdupOpt()
    C.memset(C.byref(o), 0xff, C.sizeof(o))
    L.bmh_markdup_opt_default(C.byref(o))
    assert (o.optical_distance, o.optical_max_set, o.barcode_mode, o.barcode_edits, o.barcode_max_set) == (-1, 0, 0, -1, 0)
    assert not o.rg_ids and not o.rg_lib and o.n_groups == 0
    # opt NULL is that record
    out, res = C.c_void_p(), MarkdupCounts()
    s = stream()
    assert L.bmh_bam_markdup_host(s, len(s), None, C.byref(out), C.byref(res)) == 0
    try:
        assert (C.string_at(out.value, len(s)), dict(zip(MARKDUP_COUNTS, res.counts))) == host_markdup({})
    finally:
        L.bmh_free(out)


@pytest.mark.parametrize("kw", COMBOS, ids=kw_id)
def test_optical_counting_changes_no_record_and_no_count(kw):
    recs, c = host_markdup(kw)
    base_recs, base = host_markdup(without(kw, "optical_distance"))
    assert recs == base_recs
    assert [c[k] for k in MARKDUP_COUNTS] == [base[k] for k in MARKDUP_COUNTS]
    assert without(c, *OPTICAL_COUNTS, "libraries") == without(base, "libraries")
    if "read_groups" in kw:
        assert {nm: without(v, *OPTICAL_COUNTS) for nm, v in c["libraries"].items()} == base["libraries"]


@pytest.mark.parametrize("kw", COMBOS, ids=kw_id)
def test_keys_present_and_families_agree(kw):
    c = host_markdup(kw)[1]
    want = set(MARKDUP_COUNTS)
    want |= set(OPTICAL_COUNTS) if "optical_distance" in kw else set()
    want |= {"templates_without_barcode"} if "barcode_tag" in kw else set()
    want |= set(BARCODE_GROUP_COUNTS) if "barcode_edits" in kw else set()
    want |= {"libraries"} if "read_groups" in kw else set()
    assert set(c) == want
    if "barcode_tag" in kw:                                         # (a property of the stream and the tag: no other option moves it)
        assert c["templates_without_barcode"] == host_markdup(dict(barcode_tag="RX"))[1]["templates_without_barcode"]
    if "read_groups" in kw:                                         # (the libraries' counts add up to the totals, family by family)
        for k in want - {"libraries", "templates_without_barcode"}:
            assert sum(v[k] for v in c["libraries"].values()) == c[k], k
    # the counts that say nothing about duplicates are those of the plain call
    plain = host_markdup({})[1]
    for k in ("pairs_examined", "fragments_examined", "secondary_or_supplementary", "unmapped_records", "templates"):
        assert c[k] == plain[k], k


@pytest.mark.parametrize("kw", [k for k in COMBOS if "optical_distance" not in k], ids=kw_id)
def test_sorted_file_counts_are_the_stream_calls(kw):
    bam, _index, c = bam_sorted_file(HDR, CONTIGS, stream(), host=True, markdup=True, **kw)
    assert c == host_markdup(kw)[1]
    assert bam_sorted_file(HDR, CONTIGS, host_markdup(kw)[0], host=True)[0] == bam      # (marked, then sorted: the file of the records the stream call marks)


def test_invalid_combinations():
    s = stream()
    with pytest.raises(ValueError, match=r"^bam_markdup: barcode_edits groups the barcodes that are compared: it needs barcode_tag or barcode_name$"):
        bam_markdup(s, host=True, barcode_edits=1)
    with pytest.raises(ValueError, match=r"^bam_markdup: barcode_tag and barcode_name are two sources of one barcode: give one$"):
        bam_markdup(s, host=True, barcode_tag="RX", barcode_name=True)
    with pytest.raises(ValueError, match=r"^bam_markdup: optical_max_set needs optical_distance$"):
        bam_markdup(s, host=True, optical_max_set=5)
    with pytest.raises(ValueError, match=r"^bam_markdup: barcode_max_set needs barcode_edits$"):
        bam_markdup(s, host=True, barcode_tag="RX", barcode_max_set=5)
    with pytest.raises(ValueError, match=r"^bam_sorted_file: read_groups needs markdup=True \(they decide which templates may be duplicates of each other\)$"):
        bam_sorted_file(HDR, CONTIGS, s, host=True, read_groups=GROUPS)
    with pytest.raises(ValueError, match=r"^bam_sorted_file: barcode_edits groups the barcodes that are compared: it needs barcode_tag or barcode_name$"):
        bam_sorted_file(HDR, CONTIGS, s, host=True, markdup=True, barcode_edits=1)
    with pytest.raises(ValueError, match=r"^bam_sorted_file: barcode_tag and barcode_name are two sources of one barcode: give one$"):
        bam_sorted_file(HDR, CONTIGS, s, host=True, markdup=True, barcode_tag="RX", barcode_name=True)
    with pytest.raises(ValueError, match="no read groups were given"):      # (an empty list is a table without rows, not no table)
        bam_markdup(s, host=True, read_groups=[])


def test_a_sorted_file_refuses_an_optical_distance():
    """the stand-alone file has no optical step: the record that asks for one is refused, not read past"""
    L = _sorted_file_api(_markdup_api(load_library()))
    s = stream()
    o, res = MarkdupOpt(), MarkdupCounts()
    L.bmh_markdup_opt_default(C.byref(o))
    o.optical_distance = DISTANCE
    fo = SortedOpt(1, 0, 0, 14, 0, None, C.pointer(o), None, None)
    names = (C.c_char_p * len(CONTIGS))(*[c[0].encode() for c in CONTIGS])
    lens = (C.c_int32 * len(CONTIGS))(*[c[1] for c in CONTIGS])
    bam, idx, nb, ni = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    call = lambda r: L.bmh_bam_sorted_file_host(HDR.encode(), len(CONTIGS), names, C.cast(lens, C.c_void_p), s, len(s), C.byref(fo), C.byref(bam), C.byref(nb), C.byref(idx), C.byref(ni), r)
    with_counts = C.byref(SortedResults(C.pointer(res), None, None))
    assert call(with_counts) == -2 and bam.value is None
    o.optical_distance = -1
    assert call(None) == -2 and bam.value is None                   # (marking without its counts record)
    assert call(C.byref(SortedResults())) == -2 and bam.value is None
    assert call(with_counts) == 0 and dict(zip(MARKDUP_COUNTS, res.counts)) == host_markdup({})[1]
    L.bmh_free(bam); L.bmh_free(idx)
