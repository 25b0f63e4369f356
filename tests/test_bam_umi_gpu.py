"""Barcode-aware duplicate keys on the device: test_bam_umi.py's cases and corpus through the kernels (records, counts, per-library and optical counts and the
barcode words equal the host forms'), keys whose runs of one barcode cross a 256-lane workgroup in the pair pass, the fragment pass and its max-scan, the sorted
file at several windows, reads with RX:Z comments -> marked sorted BAM end to end through align_files against the model of test_bam_umi.py applied to the output
grouped by read name (across batch cuts and a spilling run store), and the `python -m bwamem_hip.mem --barcode-tag` command with its refusals."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import common
from test_bam_dup import name_of
from test_bam_dup_gpu import _flagged, _writer_order
from test_bam_gpu import PREFIX, _reads_files
from test_bam_sort import CONTIGS, BamFile, split_records
from test_bam_umi import CORPUS, GROUPS, cases, corpus_expected, corpus_kw, corpus_stream, flags, join, sorted_file_stream, ufrag, umi_model, upair

UMI3 = (b"ACGTAC", b"ACGTAA", b"TTGACA-GGA")


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def _both(stream, **kw):
    """bam_markdup on the device, asserted equal to the host form's: bytes and every count"""
    from bwamem_hip.lib import bam_markdup
    got = bam_markdup(stream, **kw)
    assert got == bam_markdup(stream, host=True, **kw)
    return got


@pytest.mark.gpu
def test_hand_made_cases_device(hip):
    for what, stream, kw, bits, none in cases():
        got, c = _both(stream, **kw)
        assert flags(got) == bits and c["templates_without_barcode"] == none, what


@pytest.mark.gpu
@pytest.mark.parametrize("mode,groups,optical", CORPUS)
def test_device_equals_host_on_the_corpus(hip, mode, groups, optical):
    from bwamem_hip.lib import bam_dup_barcodes, bam_markdup
    stream, kw = corpus_stream(mode, groups), corpus_kw(mode, groups, optical)
    got, c = _both(stream, **kw)
    want, counts, _strings = corpus_expected(mode, groups, optical)
    assert c == counts and got == want
    src = dict(tag="RX") if mode == "tag" else dict(name=True)
    assert bam_dup_barcodes(stream, **src).tobytes() == bam_dup_barcodes(stream, host=True, **src).tobytes()
    plain_kw = {k: v for k, v in kw.items() if not k.startswith("barcode")}
    assert bam_markdup(stream, **plain_kw) == bam_markdup(stream, barcode_tag=None, **plain_kw) == bam_markdup(stream, host=True, **plain_kw)


@pytest.mark.gpu
def test_a_key_across_workgroups(hip):
    """600 pairs on one (lo, hi) and 600 fragments on one end word, three barcodes interleaved in input order, distinct scores: the run of one (key, barcode) is 200
    lanes long and the three of them lie across the 256-lane boundaries of bdp_pair_decide, bdp_run_heads and the max-scan"""
    order = [int(v) for v in np.random.default_rng(8).permutation(600)]
    # 600 distinct scores: 50 bases of quality 20 and order [k] more, spread over the bases up to 40 each
    score = {k: [40] * (v // 20) + [20 + v % 20] + [20] * (49 - v // 20) for k, v in enumerate(order)}
    best = {u: max(range(u, 600, 3), key=lambda k: order[k]) for u in range(3)}
    pairs = join([upair(b"p%03d" % k, 5000, 5400, UMI3[k % 3], q=score[k]) for k in range(600)])
    got, c = _both(pairs, barcode_tag="RX")
    assert c["duplicate_pairs"] == 597 and c["pairs_examined"] == 600 and c["records_flagged"] == 2 * 597
    assert {b"p%03d" % k for k in best.values()} == {name_of(r) for r in split_records(got)} - _flagged(got)
    assert _both(pairs)[1]["duplicate_pairs"] == 599
    frags = join([ufrag(b"f%03d" % k, 7000, UMI3[k % 3], q=score[k]) for k in range(600)])
    got, c = _both(frags, barcode_tag="RX")
    assert c["duplicate_fragments"] == 597 and c["fragments_examined"] == 600
    assert {b"f%03d" % k for k in best.values()} == {name_of(r) for r in split_records(got)} - _flagged(got)
    # both at once, a pair of one barcode only at the fragments' end: its 200 fragments all go, of the others the best stays
    mixed = join([upair(b"pp", 7000, 7400, UMI3[1])]) + frags
    got, c = _both(mixed, barcode_tag="RX")
    assert c["duplicate_fragments"] == 598 and c["duplicate_pairs"] == 0
    assert {name_of(r) for r in split_records(got)} - _flagged(got) == {b"pp", b"f%03d" % best[0], b"f%03d" % best[2]}
    # with an optical distance: a set is one barcode's 200 pairs
    named = join([upair(b"M:7:FC:1:3:%d:9" % (10 * k), 5000, 5400, UMI3[k % 3], q=score[k]) for k in range(600)])
    _got, c = _both(named, barcode_tag="RX", optical_distance=30, optical_max_set=200)
    assert (c["optical_duplicate_pairs"], c["located_pairs"], c["optical_sets_skipped"]) == (597, 600, 0)      # (members 30 apart in x: three chains of 200)
    assert _both(named, barcode_tag="RX", optical_distance=30, optical_max_set=199)[1]["optical_sets_skipped"] == 3


@pytest.mark.gpu
@pytest.mark.parametrize("window", (0, 1, 7, 100))
def test_sorted_file_device(hip, window):
    from bwamem_hip.lib import bam_sorted_file
    hdr = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:x\tLN:1\n"
    s = sorted_file_stream()
    kw = dict(markdup=True, read_groups=GROUPS, barcode_tag="RX")
    dev = bam_sorted_file(hdr, CONTIGS, s, 1, window, **kw)
    assert dev == bam_sorted_file(hdr, CONTIGS, s, 1, window, host=True, **kw)
    assert dev[2] == umi_model(s, tag="RX", read_groups=GROUPS)[1]
    if window == 7:
        name_kw = dict(markdup=True, barcode_name=True, index_format="csi")
        ns = corpus_stream("name", False)
        assert bam_sorted_file(hdr, CONTIGS, ns, 1, window, **name_kw) == bam_sorted_file(hdr, CONTIGS, ns, 1, window, host=True, **name_kw)


# ---------------------------------------------------------------------------------------------------------------- end to end

def _umi_reads(tmp_path, paired):
    """_reads_files' reads as FASTQ with RX:Z: comments; every fifth template has two copies behind all the originals (other batches): one under its own UMI, one
    under another.  Returns (path, names in input order)"""
    src = _reads_files(tmp_path, True)
    lines = open(src, "rb").read().split(b"\n")
    reads = [(lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4) if lines[i]]
    out, names = [], []
    for copy in range(3):
        for t in range(len(reads) // 2):
            if copy and t % 5 != 1:                              # (not the chimeric and random reads: those are every fifth pair from 0)
                continue
            umi = UMI3[(t + (1 if copy == 2 else 0)) % 3]
            name = b"u%d_%d" % (t, copy)
            names.append(name)
            for m in ((0, 1) if paired else (0,)):
                seq, q = reads[2 * t + m]
                out.append(b"@" + name + (b"/%d" % (m + 1) if paired else b"") + b" RX:Z:" + umi + b"\n" + seq + b"\n+\n" + q + b"\n")
    path = str(tmp_path / ("umi_pe.fq" if paired else "umi_se.fq"))
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return path, names


@pytest.mark.gpu
@pytest.mark.parametrize("paired", (False, True))
def test_reads_to_barcode_marked_bam(hip, tmp_path, monkeypatch, paired):
    from bwamem_hip.aligner import Aligner
    path, names = _umi_reads(tmp_path, paired)
    al = Aligner(PREFIX, n_threads=4)
    al.set_options(["-C"])
    monkeypatch.setenv("BMH_ALIGNER_LANES", "2")

    def run(barcode=True, **knobs):
        out, idx = io.BytesIO(), io.BytesIO()
        al.align_files(path, out=out, paired=paired, fmt="bam", sort=True, index=idx, markdup=True, sort_window=100, **(dict(barcode_tag="RX") if barcode else {}), **knobs)
        return out.getvalue(), idx.getvalue()
    base = run(batch_reads=256 if paired else 128)
    assert al.last_stats.n_batches >= 3
    counts = dict(al.markdup_counts)
    stream = _writer_order(BamFile(base[0]).stream, names)
    want, model_counts, strings = umi_model(stream, tag="RX")
    assert set(strings) == set(UMI3) and counts == model_counts and counts["templates_without_barcode"] == 0
    assert _flagged(stream) == _flagged(want)
    copies = {n for n in names if n.endswith(b"_1")}
    others = {n for n in names if n.endswith(b"_2")}
    assert len(_flagged(stream) & copies) > len(copies) // 2 > len(_flagged(stream) & others)      # a copy under its own UMI goes, one under another UMI stays
    # batch cuts and a run store that spills every run: the same file
    spill = tmp_path / "spill"; spill.mkdir()
    for knobs in (dict(batch_reads=128 if paired else 64), dict(batch_reads=256 if paired else 128, sort_mem=1, sort_tmp=str(spill))):
        assert run(**knobs) == base, knobs
        assert dict(al.markdup_counts) == counts
    assert os.listdir(spill) == []
    monkeypatch.setenv("BMH_ALIGNER_HOST_FORMAT", "1")                 # batches the host formats bring their barcode words through the host form
    assert run(batch_reads=256 if paired else 128) == base
    monkeypatch.delenv("BMH_ALIGNER_HOST_FORMAT")
    # without the option: strictly more flagged, no new count
    plain = run(barcode=False, batch_reads=256 if paired else 128)
    assert _flagged(BamFile(plain[0]).stream) > _flagged(stream) and "templates_without_barcode" not in al.markdup_counts
    # a barcode source without marking cannot be written down in the options record any more: the keywords refuse it, and the aligner stays as it was
    with pytest.raises(ValueError, match="marked"):
        al._native_aligner().set_sorted(barcode_tag="RX")
    assert run(barcode=False, batch_reads=256 if paired else 128) == plain
    # refused before anything is written
    al.close()
    al = Aligner(PREFIX, n_threads=4)                                  # (without -C)
    out = io.BytesIO()
    with pytest.raises(ValueError, match="-C"):
        al.align_files(path, out=out, paired=paired, fmt="bam", sort=True, markdup=True, barcode_tag="RX")
    with pytest.raises(ValueError, match="markdup"):
        al.align_files(path, out=out, paired=paired, fmt="bam", sort=True, barcode_name=True)
    assert out.getvalue() == b""
    al.close()


@pytest.mark.gpu
def test_mem_command(hip, tmp_path):
    path, names = _umi_reads(tmp_path, True)
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(common.GOLDEN), "..", "bwa-mem_gpu_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def mem(*args):
        return subprocess.run([sys.executable, "-m", "bwamem_hip.mem", *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    bam, met = str(tmp_path / "x.bam"), str(tmp_path / "m.txt")
    r = mem("-p", "-C", "--sort", "--markdup", "--markdup-metrics", met, "--barcode-tag", "RX", PREFIX, path, "-o", bam)
    assert r.returncode == 0, r.stderr.decode()
    with open(bam, "rb") as f:
        stream = _writer_order(BamFile(f.read()).stream, names)
    assert _flagged(stream) == _flagged(umi_model(stream, tag="RX")[0]) and _flagged(stream)
    with open(met) as f:
        assert f.read().split("\n")[1].split("\t")[-2:] == ["READ_PAIR_DUPLICATES", "PERCENT_DUPLICATION"]      # the table keeps its columns
    for args, word in ((("-p", "-C", "--sort", "--barcode-tag", "RX"), "--markdup"), (("-p", "--sort", "--markdup", "--barcode-tag", "RX"), "-C")):
        r = mem(*args, PREFIX, path, "-o", str(tmp_path / "refused.bam"))
        assert r.returncode == 2 and word in r.stderr.decode() and not os.path.exists(str(tmp_path / "refused.bam"))
