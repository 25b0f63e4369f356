"""Sort, mark duplicates and index a BAM or SAM of any aligner on the device: bmh_bam_post_file_device equals the host form byte for byte -- file,
index, counts, coverage and the words of every refusal -- on test_bam_post.py's case table and golden-set files at every batch_bytes and window; and end to end:
this aligner's own unsorted BAM and its SAM text put through the tool give the file, index, counts, metrics and coverage of its --sort --markdup --coverage run."""
import io

import numpy as np
import pytest

import common
from test_bam_post import BATCHES, CONTIGS, HEADER, WINDOWS, bam_file, golden, golden_files, post, refusal_cases, run_case, table


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def same(a, b, what):
    assert a[0] == b[0] and a[1] == b[1], what
    ra, rb = a[2], b[2]
    assert ra["counts"] == rb["counts"] and ra.get("markdup") == rb.get("markdup") and ra["header"] == rb["header"] and ra["contigs"] == rb["contigs"], what
    for k, v in rb.get("coverage", {}).items():
        assert np.array_equal(ra["coverage"][k], v), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", table(), ids=lambda c: c[0])
def test_device_equals_model_and_host(hip, tmp_path, case):
    what, records, markdup, must = case
    run_case(tmp_path, what, records, markdup, must, host=False)
    if "refused" in must:
        return
    path = str(tmp_path / "in.bam")
    for bb in BATCHES:
        for w in WINDOWS:
            kw = dict(markdup=markdup, batch_bytes=bb, sort_window=w, coverage=io.StringIO(), optical_distance=100 if markdup else None)
            same(post(path, host=False, **kw), post(path, host=True, **kw), (what, bb, w))


@pytest.mark.gpu
@pytest.mark.parametrize("bb", BATCHES)
def test_device_equals_host_on_the_golden_sets(hip, tmp_path, bb):
    for g in golden():
        # (every batch_bytes and window on the BAM; the SAM text, whose records reach the batches the same way, at the default)
        for path in golden_files(tmp_path, g)[:2 if bb is None else 1]:
            for w in WINDOWS:
                for kw in (dict(markdup=True, coverage=io.StringIO(), index_format="csi" if w == 7 else "bai"),) + ((dict(),) if w == 0 else ()):
                    same(post(path, host=False, batch_bytes=bb, sort_window=w, **kw), post(path, host=True, batch_bytes=bb, sort_window=w, **kw), (g[0], path, bb, w))
    g = max(golden(), key=lambda g: len(g[3]))
    path = golden_files(tmp_path, g)[0]
    kw = dict(markdup=True, batch_bytes=4096 if bb is None else bb, barcode_name=True, barcode_edits=None)
    spilled, held = post(path, host=False, sort_mem=1, **kw), post(path, host=True, **kw)
    assert spilled[2]["counts"].pop("spilled_runs") == spilled[2]["counts"]["batches"] and held[2]["counts"].pop("spilled_runs") == 0      # (the host form holds its records in memory)
    same(spilled, held, (g[0], "spilled"))


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(refusal_cases()[0]))
def test_refusal_messages_equal_the_host_forms(hip, tmp_path, which):
    from bwamem_hip.bam import bam_post_file
    stream, _match, kw = refusal_cases()[0][which]
    path = bam_file(tmp_path / "bad.bam", HEADER, CONTIGS, stream)
    for bb in (None, 1):
        words = []
        for host in (True, False):
            out = io.BytesIO()
            with pytest.raises(ValueError) as e:
                bam_post_file(path, out, host=host, batch_bytes=bb, **kw)
            assert out.getvalue() == b""
            words.append(str(e.value).replace("_device", "_host"))
        assert words[0] == words[1], (which, bb)


# ---------------------------------------------------------------------------------------------------------------- end to end

def _reads(tmp_path, g, n_pairs=300, L=100):
    """n_pairs pairs under distinct Illumina names (seven fields, so that the optical step has locations), every fifth repeated under a new name a few pixels away;
    a third of the templates carry an RX:Z comment"""
    from bwamem_hip import synth
    reads = synth.make_pairs(g, n_pairs, L, seed=7, sub_rate=0.01)[0]
    asc = [synth.codes_to_ascii(np.asarray(r)).tobytes() for r in reads]
    quals = [bytes(q) for q in synth.random_quals([len(a) for a in asc], seed=7)]
    umis = (b"ACGTAC", b"ACGTAA", b"TTGACA")
    out = []
    for copy in range(2):
        for t in range(n_pairs):
            if copy and t % 5:
                continue
            name = b"M1:7:FC:1:%d:%d:%d" % (1101 + t % 3, 1000 + 10 * t + 30 * copy, 2000 + 7 * t + 20 * copy)
            comment = b" RX:Z:" + umis[t % 2] if t % 3 == 0 else b""
            for m in (0, 1):
                out.append(b"@" + name + b"/%d" % (m + 1) + comment + b"\n" + asc[2 * t + m] + b"\n+\n" + quals[2 * t + m] + b"\n")
    path = str(tmp_path / "pe.fq")
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return path


@pytest.mark.gpu
def test_the_aligners_own_output_through_the_tool(hip, tmp_path):
    from bwamem_hip.aligner import Aligner
    g, idx = common.genome_and_index(20_000)
    fq = _reads(tmp_path, g)
    al = Aligner.from_memory(idx, g, n_threads=4)
    try:
        al.set_options(["-C"])
        ubam, usam = str(tmp_path / "u.bam"), str(tmp_path / "u.sam")
        with open(ubam, "wb") as f:
            al.align_files(fq, out=f, paired=True, fmt="bam")
        with open(usam, "w") as f:
            al.align_files(fq, out=f, paired=True, fmt="sam")
        for index_format in ("bai", "csi"):
            want = {k: io.StringIO() for k in ("metrics", "table", "hist", "bed")}
            out, ix = io.BytesIO(), io.BytesIO()
            al.align_files(fq, out=out, paired=True, fmt="bam", sort=True, index=ix, markdup=True, markdup_metrics=want["metrics"], optical_distance=100, barcode_tag="RX",
                           index_format=index_format, coverage=want["table"], coverage_hist=want["hist"], coverage_bed=want["bed"], coverage_bin=500)
            counts = dict(al.markdup_counts)
            assert counts["duplicate_pairs"] > 20 and counts["optical_duplicate_pairs"] > 0 and counts["templates_without_barcode"] > 0
            for src in (ubam, usam):
                got = {k: io.StringIO() for k in want}
                from bwamem_hip.bam import bam_post_file
                o, i = io.BytesIO(), io.BytesIO()
                r = bam_post_file(src, o, index=i, markdup=True, markdup_metrics=got["metrics"], optical_distance=100, barcode_tag="RX", index_format=index_format,
                                  coverage=got["table"], coverage_hist=got["hist"], coverage_bed=got["bed"], coverage_bin=500)
                assert o.getvalue() == out.getvalue() and i.getvalue() == ix.getvalue(), (src, index_format)
                assert r["markdup"] == counts and r["counts"]["bins_changed"] == 0 and r["counts"]["duplicate_flags_cleared"] == 0, (src, r["markdup"], counts)
                for k in want:
                    assert got[k].getvalue() == want[k].getvalue(), (src, k)
                assert all(np.array_equal(r["coverage"][k], v) for k, v in al.coverage.items())
        # a second run over the tool's own output gives the same file: 0x400 is cleared before the decision -- but a sorted file has the mates apart, so it is
        # refused for marking and taken for a plain sort
        sorted_path = str(tmp_path / "s.bam")
        with open(sorted_path, "wb") as f:
            f.write(out.getvalue())
        with pytest.raises(ValueError, match="--collate"):
            post(sorted_path, host=False, markdup=True)
        again = post(sorted_path, host=False, index_format="csi")
        assert again[0] == out.getvalue() and again[1] == ix.getvalue()
    finally:
        al.close()
