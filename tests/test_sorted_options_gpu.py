"""The options of sorted output as one record, on the device: over test_sorted_options' matrix the device form of bam_sorted_file gives what the host's single-feature
calls give; and the aligner's one setter and one results call on test_bam_umi_edits_gpu's reads (a few hundred pairs in several batches and windows) -- a run
with everything on equals the stand-alone post-processor on the run's own unsorted output, a refused bmh_aligner_set_sorted_output leaves the
aligner as it was, and a part the last run did not compute is refused by name.  All comparisons are exact."""
import ctypes as C
import io

import pytest

from test_sorted_options import MARKING, check_combination, marking_id, same_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.mark.parametrize("kw", MARKING, ids=marking_id)
def test_every_part_on_the_device_equals_its_single_feature_call(hip, kw):
    check_combination(kw, host=False)


def test_a_refused_record_is_worded_alike_by_both_forms(hip):
    from bwamem_hip.lib import bam_sorted_file
    from test_bam_stats import srec
    for host in (True, False):                                     # (the host form names itself, the device's windows say "sorted BAM": the words behind are the same)
        with pytest.raises(ValueError, match="(bmh_bam_sorted_file_host|sorted BAM): record 1 has an NM tag that is no count"):
            bam_sorted_file("@CO\tx\n", [("c", 1000)], srec(b"b", pos=20, tag=b"NMZ1\0") + srec(b"ok"), host=host, window=1, coverage={}, stats={})


def test_the_aligners_one_setter_and_one_results_call(hip, tmp_path, monkeypatch):
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import SortedOpt, _err, bam_post
    from test_bam_umi_edits_gpu import PREFIX, _edited_reads
    path, _names = _edited_reads(tmp_path)
    al = Aligner(PREFIX, n_threads=4)
    al.set_options(["-C"])
    monkeypatch.setenv("BMH_ALIGNER_LANES", "2")
    try:
        # one run with everything on = the post-processor on the run's own unsorted output
        everything = dict(markdup=True, optical_distance=100, barcode_tag="RX", barcode_edits=1, index_format="csi", csi_min_shift=12)
        out, idx = io.BytesIO(), io.BytesIO()
        al.align_files(path, out=out, paired=True, fmt="bam", sort=True, index=idx, sort_window=100, batch_reads=256, coverage=io.StringIO(), coverage_bed=io.StringIO(), coverage_bin=500, stats=io.StringIO(),
                       insert_cap=1000, **everything)
        assert al.last_stats.n_batches >= 3
        counts, cov, st = dict(al.markdup_counts), al.coverage, al.stats
        assert counts["records_flagged"] > 0 and counts["pair_barcodes_inferred"] < counts["pair_barcodes_observed"] and "optical_duplicate_pairs" in counts
        unsorted = str(tmp_path / "u.bam")
        with open(unsorted, "wb") as f:
            al.align_files(path, out=f, paired=True, fmt="bam", batch_reads=256)
        pieces = []
        r = bam_post(unsorted, pieces.append, window=100, coverage=dict(bin=500), stats=dict(insert_cap=1000), **everything)
        assert b"".join(pieces) == out.getvalue() and r["index"] == idx.getvalue()
        assert r["markdup"] == counts and same_arrays(r["coverage"], cov) and same_arrays(r["stats"], st)
        assert int(st["flag"][0, 4]) == counts["records_flagged"] and len(cov["bin_sum"]) > 1

        # the handle itself, without the layer that sets everything anew before each run
        nat = al._native_aligner()

        def run():
            got = []
            nat.run_files(path, None, True, lambda mv: got.append(bytes(mv)), batch_reads=256, n_lanes=2, n_threads=4)
            return b"".join(got), nat.sort_index(0), nat.sorted_results()
        nat.set_sorted(markdup=True, barcode_tag="RX", barcode_edits=1, window=100, stats=dict(insert_cap=1000))
        before = run()
        assert set(before[2]) == {"markdup_counts", "markdup_library_counts", "markdup_times", "markdup_barcode_counts", "markdup_barcode_group_counts", "stats", "stats_ms"}
        assert before[2]["markdup_counts"]["records_flagged"] == counts["records_flagged"] and before[2]["markdup_library_counts"] == [] and before[2]["stats_ms"][1] >= 3
        for kw, words in ((dict(markdup=True, barcode_edits=1), "barcode_tag or barcode_name"), (dict(coverage={}, index_format="csi", csi_min_shift=9), "10 .. 24"),
                          (dict(barcode_tag="RX"), "marked"), (dict(markdup=True, read_groups=[("a", "l")]), "read groups come from")):
            with pytest.raises(ValueError, match=words):
                nat.set_sorted(**kw)
        # ... and one the keywords cannot catch: the record as a C caller writes it, good parts in front of the bad one
        L = hip.load_library()
        opt = SortedOpt(0, 5, 1, 9, 1, None, None, None, None)
        assert L.bmh_aligner_set_sorted_output(nat.handle, C.byref(opt)) == -2 and "min_shift" in _err(L)
        after = run()
        assert after[0] == before[0] and after[1] == before[1] and after[2]["markdup_counts"] == before[2]["markdup_counts"] and same_arrays(after[2]["stats"], before[2]["stats"])
        # a part the last run did not compute is refused by name
        with pytest.raises(ValueError, match=r"no run has computed coverage \(or the last one failed before its file was complete\)"):
            nat.sorted_results("coverage")
        with pytest.raises(ValueError, match=r"no run has counted optical duplicates \(or the last one failed before its file was complete\)"):
            nat.sorted_results("optical")
        nat.set_output("bam_sorted", 1)                           # the default record: nothing of the options stays on, and no run has been made under it
        with pytest.raises(ValueError, match=r"no run has marked duplicates \(or the last one failed before its file was complete\)"):
            nat.sorted_results("markdup")
        assert nat.sorted_results() == {}
        nat.set_output("sam", 1)
    finally:
        al.close()
