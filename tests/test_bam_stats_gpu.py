"""Flagstat, idxstats, alignment summary and insert sizes on the device: the table and the synthetic stream of test_bam_stats.py through the
kernel at both insert caps (device integers equal the host form's and the model's), the edges of a block of 256 lanes, contigs that change inside a block, the
refusals word for word, the windows of the sorted file's merge beside duplicate marking and coverage, and reads -> sorted, marked BAM with its three texts end to
end against the model applied to the records of the file just written -- and the same texts from `bwamem_hip.bam` on that run's unsorted BAM."""
import io

import numpy as np
import pytest

from test_bam_dup_gpu import _dup_reads
from test_bam_gpu import PREFIX
from test_bam_sort import BamFile, py_sort, split_records
from test_bam_stats import (REFUSED, WORDS, cached_model, corpus, cut, equal, flagstat_by_model, idxstats_by_model, model, srec, stats_by_model, synthetic)


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.mark.gpu
def test_device_equals_host_and_model(hip):
    from bwamem_hip.lib import bam_stats
    for what, nc, stream, cap in corpus():
        want = cached_model(what, stream, nc, cap)
        if isinstance(want, tuple):
            with pytest.raises(ValueError) as e:
                bam_stats(stream, nc, cap)
            assert str(e.value) == "bmh_bam_stats: bmh_bam_stats_device: record %d %s" % (want[1], WORDS[want[2]]), what
            continue
        got = bam_stats(stream, nc, cap)
        assert equal(got, want) and equal(got, bam_stats(stream, nc, cap, host=True)), (what, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257])
def test_block_edges(hip, n):
    from bwamem_hip.lib import bam_stats
    nc, s = synthetic(n, 21)
    assert len(split_records(s)) == n
    for stream in (s, py_sort(s)):
        assert equal(bam_stats(stream, nc, 4), model(stream, nc, 4)), n


@pytest.mark.gpu
def test_contigs_inside_a_block(hip):
    """a stream on one contig (one atomic per block and kind), a contig change inside a block, and contigs that alternate lane by lane with records without one"""
    from bwamem_hip.lib import bam_stats
    one = b"".join(srec(b"a%d" % i, 0, i, 0x4 if i % 9 == 0 else 0) for i in range(600))
    change = b"".join(srec(b"b%d" % i, 0 if i < 300 else 2, i, 0x1 | 0x4 | 0x80 if i % 7 == 0 else 0) for i in range(600))
    mixed = b"".join(srec(b"c%d" % i, i % 4 - 1, i if i % 4 else -1, 0x4 if i % 5 == 0 else 0) for i in range(600))
    for what, s in (("one", one), ("change", change), ("mixed", mixed)):
        got = bam_stats(s, 3)
        assert equal(got, model(s, 3)), what
        assert int(got["contig_mapped"].sum() + got["contig_unmapped"].sum() + got["unplaced"][0]) == 600
    assert bam_stats(one, 3)["contig_mapped"].tolist() == [600 - 67, 0, 0] and bam_stats(change, 3)["contig_unmapped"].tolist() == [43, 0, 43]


@pytest.mark.gpu
def test_refusals_on_the_device(hip):
    """the device names the same index and says the same words as the host; of two refusable records in one stream -- the later one placed first in its block --
    the earlier one is named"""
    from bwamem_hip.lib import bam_stats
    many = b"".join(srec(b"r%03d" % i, 0, 10 + i) for i in range(300))
    for what, r, code in REFUSED:
        r = cut(r) if what == "bases past the record" else r
        stream = many + r + srec(b"ok") * 211 + srec(b"late", tag=b"NMZ1\0") + srec(b"ok")          # records 300 and 512: the second is lane 0 of the third block
        assert len(split_records(stream)) == 514
        msgs = []
        for host in (False, True):
            with pytest.raises(ValueError) as e:
                bam_stats(stream, 2, host=host)
            msgs.append(str(e.value))
        assert msgs[0] == "bmh_bam_stats: bmh_bam_stats_device: record 300 " + WORDS[code] and msgs[1] == msgs[0].replace("_device", "_host"), what
    from bwamem_hip.lib import bam_sorted_file
    with pytest.raises(ValueError, match="sorted BAM: record 300 has an NM tag that is no count"):
        bam_sorted_file("@CO\tx\n", [("c", 1000)], many + srec(b"b", pos=400, tag=b"NMZ1\0") + srec(b"c", pos=500), stats={})


@pytest.mark.gpu
@pytest.mark.parametrize("window", [0, 1, 7, 25])
def test_windows_of_the_device_merge(hip, window):
    """beside duplicate marking and coverage: the bytes, the counts and the coverage are those of the run without statistics, the statistics the host's and the
    model's over the file's records with their final 0x400 flags"""
    from bwamem_hip.lib import bam_sorted_file
    from test_bam_dup import one_key
    nc, s = synthetic(400, 5)
    contigs = [("c%d" % i, 3000) for i in range(nc)]
    bam, bai, got = bam_sorted_file("@CO\tx\n", contigs, s, 1, window, stats=dict(insert_cap=4))
    assert (bam, bai) == bam_sorted_file("@CO\tx\n", contigs, s, 1, window) and equal(got, model(BamFile(bam).stream, nc, 4))
    assert equal(got, bam_sorted_file("@CO\tx\n", contigs, s, 1, window, host=True, stats=dict(insert_cap=4))[2])
    dups = one_key(40)
    contigs = [("a", 1000), ("b", 2000)]
    plain = bam_sorted_file("@CO\tx\n", contigs, dups, 1, window, markdup=True, coverage={})
    bam, bai, counts, cov, got = bam_sorted_file("@CO\tx\n", contigs, dups, 1, window, markdup=True, coverage={}, stats={})
    assert (bam, bai, counts) == plain[:3] and all(np.array_equal(cov[k], plain[3][k]) for k in cov)
    assert counts["records_flagged"] > 0 and int(got["flag"][0][4]) == counts["records_flagged"] and equal(got, model(BamFile(bam).stream, 2))
    assert equal(got, bam_sorted_file("@CO\tx\n", contigs, dups, 1, window, host=True, markdup=True, coverage={}, stats={})[4])


@pytest.mark.gpu
def test_reads_to_sorted_bam_with_statistics(hip, tmp_path):
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.bam import bam_post_file
    reads = _dup_reads(tmp_path, True)[0]
    al = Aligner(PREFIX, n_threads=4)
    try:
        def run(**kw):
            out, idx = io.BytesIO(), io.BytesIO()
            al.align_files(reads, out=out, fmt="bam", sort=True, index=idx, paired=True, markdup=True, batch_reads=256, sort_window=7, **kw)
            return out.getvalue(), idx.getvalue()
        texts = [io.StringIO() for _ in range(3)]
        plain = run()
        assert run(flagstat=texts[0], idxstats=texts[1], stats=texts[2]) == plain
        assert al.last_stats.n_batches >= 3 and al.markdup_counts["records_flagged"] > 0
        want = model(BamFile(plain[0]).stream, len(al.contigs))
        assert equal(al.stats, want)
        assert int(want["flag"][0][4]) == al.markdup_counts["records_flagged"] and int(want["insert_hist"].sum()) > 50 and int(want["summary"][12]) > 100
        want_texts = [flagstat_by_model(want), idxstats_by_model(want, al.contigs), stats_by_model(want, al.contigs)]
        assert [t.getvalue() for t in texts] == want_texts
        small = io.StringIO()
        assert run(stats=small, insert_cap=4) == plain and small.getvalue() == stats_by_model(model(BamFile(plain[0]).stream, len(al.contigs), 4), al.contigs)
        assert run() == plain                                                    # switched off again: the next run launches nothing more and writes the same file
        ubam = str(tmp_path / "u.bam")
        with open(ubam, "wb") as f:
            al.align_files(reads, out=f, fmt="bam", paired=True, batch_reads=256)
        for host in (False, True):
            got, o, i = [io.StringIO() for _ in range(3)], io.BytesIO(), io.BytesIO()
            r = bam_post_file(ubam, o, index=i, host=host, markdup=True, sort_window=7, flagstat=got[0], idxstats=got[1], stats=got[2])
            assert (o.getvalue(), i.getvalue()) == plain and [t.getvalue() for t in got] == want_texts and equal(r["stats"], want), host
    finally:
        al.close()
