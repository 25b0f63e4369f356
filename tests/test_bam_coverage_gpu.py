"""Coverage depth on the device: the table and the synthetic stream of test_bam_coverage.py through the kernels at every (tile, bin), with
deletions off and on and min_mapq 0 and 20 (device integers equal the host form's and the model's), the windows of the sorted file's merge, reads -> sorted,
marked BAM with its coverage end to end against the model applied to the records of the file just written, and marked duplicates counted out."""
import io

import numpy as np
import pytest

from test_bam_coverage import GRID, MAX_BINS, bed_text, check_must, corpus, equal, hist_text, model, n_bins, synthetic, table_text
from test_bam_dup import golden_doubled
from test_bam_dup_gpu import _dup_reads
from test_bam_gpu import PREFIX
from test_bam_sort import BamFile, golden_streams


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.fixture(scope="module")
def al(hip):
    from bwamem_hip.aligner import Aligner
    a = Aligner(PREFIX, n_threads=4)
    yield a
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("min_mapq", [0, 20])
@pytest.mark.parametrize("deletions", [False, True])
def test_device_equals_host(hip, deletions, min_mapq):
    """the 1 100-read stack (equal addresses, depth beyond the last exact bin), the contig of 2^31 - 1 bases and the 1000M read at tile 64 among them"""
    from bwamem_hip.lib import bam_coverage
    for what, lens, stream, kw, must in corpus():
        if not deletions and not min_mapq:                                  # the case under its own keywords: what the table spells out
            check_must(what, bam_coverage(stream, lens, **kw), must)
        for tile, bin in GRID:
            opt = dict(min_mapq=min_mapq, deletions=deletions, bin=bin, tile=tile)
            if n_bins(lens, bin) >= MAX_BINS:
                with pytest.raises(ValueError, match="fewer than 2\\^28"):
                    bam_coverage(stream, lens, **opt)
                continue
            got = bam_coverage(stream, lens, **opt)
            assert equal(got, bam_coverage(stream, lens, host=True, **opt)), (what, opt)
            if n_bins(lens, bin) < 100_000:
                assert equal(got, model(what, stream, lens, min_mapq, deletions, bin)), (what, opt)


@pytest.mark.gpu
def test_refusals_on_the_device(hip):
    from bwamem_hip.lib import bam_coverage
    from test_bam_coverage import placeholder
    from test_bam_dup import rec
    a = rec(b"a", 0, 10, 0)
    many = b"".join(rec(b"r%03d" % i, 0, 10 + i, 0) for i in range(300))
    for stream, lens, msg in ((a + rec(b"b", 0, 9, 0), [100], "bmh_bam_coverage_device: record 1 lies before record 0: coverage takes records in coordinate order"),
                              (many + rec(b"b", 0, 400, 0) + rec(b"c", 0, 401, 0), [400], r"bmh_bam_coverage_device: record 300 begins outside its contig \(pos is negative or not below the contig's length\)"),
                              (many + placeholder(pos=350) + rec(b"c", 0, 900, 0), [500], r"bmh_bam_coverage_device: record 300 holds the long-CIGAR placeholder \(its operations are in its CG tag\)")):
        with pytest.raises(ValueError, match=msg):
            bam_coverage(stream, lens)
    # two refusals in one stream: the first record refused is the one named, whatever its kind, as on the host
    for stream, lens, msg in ((many + rec(b"b", 0, 400, 0) + rec(b"c", 0, 5, 0), [400], "record 300 begins outside its contig"),
                              (many + placeholder(pos=350) + rec(b"c", 0, 5, 0), [500], "record 300 holds the long-CIGAR placeholder"),
                              (many + rec(b"c", 0, 5, 0) + rec(b"b", 0, 400, 0), [400], "record 300 lies before record 299")):
        with pytest.raises(ValueError, match=msg):
            bam_coverage(stream, lens)
        with pytest.raises(ValueError, match=msg):
            bam_coverage(stream, lens, host=True)
    got = bam_coverage(a + placeholder(False), [200])
    assert [int(got["n_reads"][0]), int(got["cov_bases"][0])] == [2, 50]


@pytest.mark.gpu
def test_equal_address_combining_changes_nothing(hip):
    """the lanes of a wave that hold one position add once (the stack of 1 100, the dense third of the synthetic stream); with the combining off every lane adds"""
    from bwamem_hip.lib import bam_coverage
    L = hip.load_library()
    for what, lens, stream, _kw, _must in corpus():
        if what not in ("1100 identical reads", "synthetic"):
            continue
        want = bam_coverage(stream, lens, bin=7, tile=64)
        try:
            L.bmh_tune_set(b"COV_COMBINE", 0, 0)
            assert equal(bam_coverage(stream, lens, bin=7, tile=64), want), what
        finally:
            L.bmh_tune_set(b"COV_COMBINE", 0, 1)
        assert equal(want, model(what, stream, lens, 0, False, 7)), what


@pytest.mark.gpu
@pytest.mark.parametrize("window", [1, 7, 25, 0])
def test_windows_of_the_device_merge(hip, window):
    """the carry across the windows of the merge: events kept behind the frontier, the stack of 1 100 cut inside, a contig's edge between two windows"""
    from bwamem_hip.lib import bam_sorted_file
    for what, lens, stream, kw, _must in corpus():
        if max(lens) >= 1 << 29 or (window == 1 and len(stream) > 100_000 and what != "synthetic"):
            continue
        contigs = [("c%d" % i, l) for i, l in enumerate(lens)]
        opt = dict(min_mapq=kw.get("min_mapq", 0), deletions=kw.get("deletions", False), bin=7, tile=kw.get("tile", 64))
        bam, bai, got = bam_sorted_file("@CO\tx\n", contigs, stream, 1, window, coverage=opt)
        assert equal(got, model(what, stream, lens, opt["min_mapq"], opt["deletions"], 7)), (what, window)
        if what == "synthetic":
            assert (bam, bai) == bam_sorted_file("@CO\tx\n", contigs, stream, 1, window)


# ---------------------------------------------------------------------------------------------------------------- end to end

def _run(al, path, cov=True, **kw):
    out, idx, texts = io.BytesIO(), io.BytesIO(), [io.StringIO(), io.StringIO(), io.StringIO()]
    if cov:
        kw.update(coverage=texts[0], coverage_hist=texts[1], coverage_bed=texts[2], coverage_bin=100)
    al.align_files(path, out=out, fmt="bam", sort=True, index=idx, **kw)
    return out.getvalue(), idx.getvalue(), [t.getvalue() for t in texts]


def _file_model(what, al, bam, **kw):
    lens = [l for _n, l in al.contigs]
    return model(what, BamFile(bam).stream, lens, kw.get("min_mapq", 0), kw.get("deletions", False), 100)


@pytest.fixture(scope="module")
def dup_reads(tmp_path_factory):
    return _dup_reads(tmp_path_factory.mktemp("cov"), True)[0]


@pytest.fixture(scope="module")
def plain_run(al, dup_reads):
    """the marked, sorted file and its index without the coverage options"""
    bam, bai, _t = _run(al, dup_reads, cov=False, paired=True, markdup=True, batch_reads=256)
    return bam, bai


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [dict(sort_window=1), dict(sort_window=7), dict(), dict(sort_window=7, sort_mem=1)], ids=["window 1", "window 7", "default window", "every run spilled"])
def test_reads_to_sorted_bam_with_coverage(al, dup_reads, plain_run, tmp_path, knobs):
    if "sort_mem" in knobs:
        knobs = dict(knobs, sort_tmp=str(tmp_path))
    bam, bai, texts = _run(al, dup_reads, paired=True, markdup=True, batch_reads=256, **knobs)
    assert al.last_stats.n_batches >= 3 and al.markdup_counts["records_flagged"] > 0
    assert (bam, bai) == (plain_run if not knobs else _run(al, dup_reads, cov=False, paired=True, markdup=True, batch_reads=256, **knobs)[:2])      # the same run without the coverage options
    want = _file_model("marked", al, bam)
    assert equal(al.coverage, want)
    assert int(want["n_reads"].sum()) > 500 and int(want["max_depth"].max()) >= 3
    assert texts == [table_text(want, al.contigs), hist_text(want), bed_text(want, al.contigs, 100)]


@pytest.mark.gpu
def test_coverage_keywords_and_read_groups(al, dup_reads, plain_run):
    bam, _bai, _t = _run(al, dup_reads, paired=True, markdup=True, batch_reads=256, coverage_min_mapq=20, coverage_deletions=True, sort_window=7)
    assert BamFile(bam).stream == BamFile(plain_run[0]).stream              # (another window: other members, the same records)
    assert equal(al.coverage, _file_model("marked, mapq 20, deletions", al, bam, min_mapq=20, deletions=True))
    _run(al, dup_reads, paired=True, markdup=True, batch_reads=256, coverage_min_mapq=61, sort_window=7)      # (no mapq goes beyond 60: nothing counts)
    assert int(al.coverage["n_reads"].sum()) == 0 and int(al.coverage["hist"][0]) == sum(l for _n, l in al.contigs) and int(_file_model("marked", al, bam)["n_reads"].sum()) > 500
    # over read groups the coverage is the whole file's: two libraries of the same reads, duplicates marked within each
    out, idx, table = io.BytesIO(), io.BytesIO(), io.StringIO()
    al.align_groups([("@RG\\tID:a\\tLB:l1", dup_reads, None), ("@RG\\tID:b\\tLB:l2", dup_reads, None)], out=out, paired=True, fmt="bam", sort=True, index=idx, markdup=True,
                    batch_reads=256, sort_window=7, coverage=table, coverage_bed=io.StringIO(), coverage_bin=100)
    want = _file_model("two groups", al, out.getvalue())
    assert equal(al.coverage, want) and table.getvalue() == table_text(want, al.contigs)
    single = _file_model("marked", al, plain_run[0])
    assert [int(v) for v in want["sum_depth"]] == [2 * int(v) for v in single["sum_depth"]]
    # switched off again: the next run has no coverage and the file is the plain one
    bam2, bai2, _t = _run(al, dup_reads, cov=False, paired=True, markdup=True, batch_reads=256)
    assert (bam2, bai2) == plain_run


@pytest.mark.gpu
def test_duplicates_are_counted_out(hip):
    """the golden records doubled: marked, the copies are out and the depth is that of the undoubled records; unmarked, it is twice that"""
    from bwamem_hip.lib import bam_sorted_file
    seen = 0
    for (what, contigs, once), (what2, contigs2, twice) in zip(golden_streams(), golden_doubled()):
        assert contigs == contigs2
        one_marked = bam_sorted_file("@CO\tx\n", contigs, once, 1, 7, markdup=True, coverage={})[3]
        one_plain = bam_sorted_file("@CO\tx\n", contigs, once, 1, 7, coverage={})[2]
        two_marked = bam_sorted_file("@CO\tx\n", contigs, twice, 1, 7, markdup=True, coverage={})[3]
        two_plain = bam_sorted_file("@CO\tx\n", contigs, twice, 1, 7, coverage={})[2]
        assert np.array_equal(two_marked["sum_depth"], one_marked["sum_depth"]) and np.array_equal(two_marked["n_reads"], one_marked["n_reads"]), what
        assert np.array_equal(two_plain["sum_depth"], 2 * one_plain["sum_depth"]), what
        seen += int(one_plain["sum_depth"].sum()) > 0
    assert seen >= 3
