"""Barcodes grouped within an edit distance on the device: test_bam_umi_edits.py's cases and corpus through the kernels (records, counts, per-library counts and
the packed words equal the host forms'), one key whose chain of 70 barcodes spans more than a wave and two 256-lane boundaries in both passes, with the cap just
below its distinct count, a few thousand small keys across the compaction's blocks, the sorted file, reads with RX:Z comments -> marked sorted BAM end to end
through align_files against the model applied to the output grouped by read name (across batch cuts, a spilling run store and host-formatted batches), and the
`python -m bwamem_hip.mem --barcode-edits` command with its refusals."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import common
from test_bam_dup import name_of, pair
from test_bam_dup_gpu import _flagged, _writer_order
from test_bam_gpu import PREFIX
from test_bam_sort import CONTIGS, BamFile, split_records
from test_bam_umi import GROUPS, flags, join, ufrag, upair, with_aux, z
from test_bam_umi_gpu import UMI3, _umi_reads
from test_bam_umi_edits import (CORPUS, GROUP_KEYS, V21, cases, corpus_expected, corpus_kw, corpus_stream, edits_model, model_kw, one_key_stream, optical_stream,
                                sorted_file_stream)


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
    from bwamem_hip.lib import bam_dup_barcodes, bam_markdup
    for what, stream, kw, bits, grp in cases():
        got, c = _both(stream, **kw)
        assert flags(got) == bits and tuple(c[k] for k in GROUP_KEYS) == grp, what
    s5, _chain = one_key_stream(5)
    for cap in (4, 5, 6):
        _both(s5, barcode_tag="RX", barcode_edits=1, barcode_max_set=cap)
    for D, want in ((10, (1, 1)), (3, (1, 0))):
        _g, c = _both(optical_stream(), barcode_tag="RX", barcode_edits=1, optical_distance=D)
        assert (c["duplicate_pairs"], c["optical_duplicate_pairs"]) == want
    # a value that does not pack: by its record's index, as the host form says it
    good, p = upair(b"g", 100, 300, b"AC"), pair(b"b", 1, 100, 0, 1, 251, 1)
    for value in (V21 + b"A", b"acgt", b"ACGU"):
        bad = join([good, good, [with_aux(p[0], z(b"RX", value)), p[1]]])
        for fn in (lambda: bam_markdup(bad, barcode_tag="RX", barcode_edits=1), lambda: bam_dup_barcodes(bad, tag="RX", edits=True)):
            with pytest.raises(ValueError, match="record 4 .*does not pack"):
                fn()
        _both(bad, barcode_tag="RX")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,groups", CORPUS)
def test_device_equals_host_on_the_corpus(hip, mode, groups):
    from bwamem_hip.lib import bam_dup_barcodes, bam_markdup
    stream = corpus_stream(mode, groups)
    for N in (1, 0):
        kw = corpus_kw(mode, groups, N)
        got, c = _both(stream, **kw)
        want, counts, _strings = corpus_expected(mode, groups, N)
        assert c == counts and got == want
    src = dict(tag="RX") if mode == "tag" else dict(name=True)
    assert bam_dup_barcodes(stream, edits=True, **src).tobytes() == bam_dup_barcodes(stream, host=True, edits=True, **src).tobytes()
    exact_kw = {k: v for k, v in kw.items() if k != "barcode_edits"}
    assert got == bam_markdup(stream, **exact_kw)[0]                   # N = 0 on the device: the exact mode's bytes
    if groups:
        _both(stream, optical_distance=25, optical_max_set=8, **corpus_kw(mode, groups, 1))


def _chain(n=70):
    """n barcodes of 12 symbols, each one edit from the next: step k moves place k % 12 on to its next symbol; and two barcodes far from all of them"""
    out = []
    for k in range(n):
        out.append(bytes(b"ACGTN-+"[sum(1 for j in range(k) if j % 12 == i)] for i in range(12)))
    assert len(set(out)) == n and all(sum(a != b for a, b in zip(out[k], out[k + 1])) == 1 for k in range(n - 1))
    return out + [b"+A+A+A+A+A+A", b"-C-C-C-C-C-C"]


@pytest.mark.gpu
def test_a_key_across_workgroups(hip):
    """600 pairs on one (lo, hi) and 600 fragments on one end word under 72 barcodes interleaved in input order -- a chain of 70, each one edit from the next, and
    two far from it --, distinct scores: the key's members span more than a wave, its elements two 256-lane boundaries, and the model's survivor of each of the
    three components is expected.  With the cap just below the distinct count the key is skipped and the exact mode's flags are expected"""
    umis = _chain()
    order = [int(v) for v in np.random.default_rng(8).permutation(600)]
    score = {k: [40] * (v // 20) + [20 + v % 20] + [20] * (49 - v // 20) for k, v in enumerate(order)}      # 600 distinct scores
    best = [max((k for k in range(600) if k % 72 in comp), key=lambda k: order[k]) for comp in (range(70), (70,), (71,))]
    pairs = join([upair(b"p%03d" % k, 5000, 5400, umis[k % 72], q=score[k]) for k in range(600)])
    kw = dict(barcode_tag="RX", barcode_edits=1)
    got, c = _both(pairs, **kw)
    want, counts, _s = edits_model(pairs, **model_kw(kw))
    assert got == want and c == counts
    assert c["duplicate_pairs"] == 597 and (c["pair_barcodes_observed"], c["pair_barcodes_inferred"], c["barcode_keys_skipped"]) == (72, 3, 0)
    assert {b"p%03d" % k for k in best} == {name_of(r) for r in split_records(got)} - _flagged(got)
    got, c = _both(pairs, barcode_max_set=71, **kw)
    assert got == _both(pairs, barcode_tag="RX")[0] and (c["pair_barcodes_observed"], c["pair_barcodes_inferred"], c["barcode_keys_skipped"]) == (72, 72, 3)
    assert c["duplicate_pairs"] == 600 - 72
    assert _both(pairs, barcode_max_set=72, **kw)[1]["barcode_keys_skipped"] == 0
    frags = join([ufrag(b"f%03d" % k, 7000, umis[k % 72], q=score[k]) for k in range(600)])
    got, c = _both(frags, **kw)
    want, counts, _s = edits_model(frags, **model_kw(kw))
    assert got == want and c == counts and c["duplicate_fragments"] == 597
    assert {b"f%03d" % k for k in best} == {name_of(r) for r in split_records(got)} - _flagged(got)
    got, c = _both(frags, barcode_max_set=71, **kw)
    assert got == _both(frags, barcode_tag="RX")[0] and c["barcode_keys_skipped"] == 1 and c["duplicate_fragments"] == 600 - 72
    # both at once, a pair in the middle of the chain at the fragments' end: the chain's fragments all go, of the two others the best stays
    mixed = join([upair(b"pp", 7000, 7400, umis[35])]) + frags
    got, c = _both(mixed, **kw)
    assert c["duplicate_fragments"] == 598 and c["duplicate_pairs"] == 0
    assert {name_of(r) for r in split_records(got)} - _flagged(got) == {b"pp", b"f%03d" % best[1], b"f%03d" % best[2]}


@pytest.mark.gpu
def test_many_small_keys(hip):
    """3000 keys of 2 to 5 distinct barcodes, some of them neighbours: the heads, their scans and the compaction across blocks"""
    rng = np.random.default_rng(3)
    tpls = []
    for key in range(3000):
        base = bytearray(rng.choice(list(b"ACGT"), size=8).tolist())
        for j in range(int(rng.integers(2, 6))):
            u = bytearray(base)
            if j:
                for _ in range(int(rng.integers(1, 3))):
                    u[int(rng.integers(0, 8))] = b"ACGT"[int(rng.integers(0, 4))]
            for copy in range(int(rng.integers(1, 3))):
                tpls.append(upair(b"k%d_%d_%d" % (key, j, copy), 1000 + 3 * key, 1400 + 3 * key, bytes(u), q=int(rng.integers(15, 40)), rg=GROUPS[key % 3][0]))
            if rng.integers(0, 3) == 0:
                tpls.append(ufrag(b"f%d_%d" % (key, j), 1000 + 3 * key, bytes(u), q=int(rng.integers(15, 40)), rg=GROUPS[key % 3][0]))
    order = rng.permutation(len(tpls))
    s = join([tpls[int(i)] for i in order])
    kw = dict(barcode_tag="RX", barcode_edits=1, read_groups=GROUPS)
    got, c = _both(s, **kw)
    want, counts, _s = edits_model(s, **model_kw(kw))
    assert got == want and c == counts
    assert c["pair_barcodes_observed"] > c["pair_barcodes_inferred"] > 3000 and c["barcode_keys_skipped"] == 0
    got, c = _both(s, barcode_max_set=3, **kw)                          # the keys of 4 and 5 are skipped, the others clustered
    want, counts, _s = edits_model(s, **model_kw(dict(kw, barcode_max_set=3)))
    assert got == want and c == counts and c["barcode_keys_skipped"] > 100


@pytest.mark.gpu
@pytest.mark.parametrize("window", (0, 7))
def test_sorted_file_device(hip, window):
    from bwamem_hip.lib import bam_sorted_file
    hdr = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:x\tLN:1\n"
    s = sorted_file_stream()
    kw = dict(markdup=True, read_groups=GROUPS, barcode_tag="RX", barcode_edits=1)
    dev = bam_sorted_file(hdr, CONTIGS, s, 1, window, **kw)
    assert dev == bam_sorted_file(hdr, CONTIGS, s, 1, window, host=True, **kw)
    assert dev[2] == edits_model(s, 1, tag="RX", read_groups=GROUPS)[1]
    if window == 7:
        name_kw = dict(markdup=True, barcode_name=True, barcode_edits=2, index_format="csi")
        ns = corpus_stream("name", False)
        assert bam_sorted_file(hdr, CONTIGS, ns, 1, window, **name_kw) == bam_sorted_file(hdr, CONTIGS, ns, 1, window, host=True, **name_kw)


# ---------------------------------------------------------------------------------------------------------------- end to end

def _edited_reads(tmp_path):
    """test_bam_umi_gpu._umi_reads' pairs, and behind them a third copy of every fifth template under a barcode one edit from its own"""
    path, names = _umi_reads(tmp_path, True)
    lines = open(path, "rb").read().split(b"\n")
    out = []
    for i in range(0, len(lines) - 1, 4):
        head = lines[i]
        if not head.startswith(b"@u") or b"_0/" not in head:
            continue
        t = int(head[2:head.index(b"_")])
        if t % 5 != 1:
            continue
        name, mate = b"u%d_3" % t, head[head.index(b"/"):head.index(b" ")]
        if mate == b"/1":
            names.append(name)
        out.append(b"@" + name + mate + b" RX:Z:N" + UMI3[t % 3][1:] + b"\n" + lines[i + 1] + b"\n+\n" + lines[i + 3] + b"\n")
    assert out
    with open(path, "ab") as f:
        f.write(b"".join(out))
    return path, names


@pytest.mark.gpu
def test_reads_to_edit_grouped_bam(hip, tmp_path, monkeypatch):
    from bwamem_hip.aligner import Aligner
    path, names = _edited_reads(tmp_path)
    al = Aligner(PREFIX, n_threads=4)
    al.set_options(["-C"])
    monkeypatch.setenv("BMH_ALIGNER_LANES", "2")

    def run(**knobs):
        out, idx = io.BytesIO(), io.BytesIO()
        al.align_files(path, out=out, paired=True, fmt="bam", sort=True, index=idx, markdup=True, sort_window=100, **knobs)
        return out.getvalue(), idx.getvalue()
    base = run(barcode_tag="RX", barcode_edits=1, batch_reads=256)
    assert al.last_stats.n_batches >= 3
    counts = dict(al.markdup_counts)
    stream = _writer_order(BamFile(base[0]).stream, names)
    want, model_counts, strings = edits_model(stream, 1, tag="RX")
    assert counts == model_counts and counts["templates_without_barcode"] == 0 and counts["pair_barcodes_inferred"] < counts["pair_barcodes_observed"]
    assert _flagged(stream) == _flagged(want)
    # batch cuts, a run store that spills every run, batches the host formats: the same file
    spill = tmp_path / "spill"; spill.mkdir()
    for knobs in (dict(batch_reads=128), dict(batch_reads=256, sort_mem=1, sort_tmp=str(spill))):
        assert run(barcode_tag="RX", barcode_edits=1, **knobs) == base, knobs
        assert dict(al.markdup_counts) == counts
    assert os.listdir(spill) == []
    monkeypatch.setenv("BMH_ALIGNER_HOST_FORMAT", "1")
    assert run(barcode_tag="RX", barcode_edits=1, batch_reads=256) == base
    assert dict(al.markdup_counts) == counts
    monkeypatch.delenv("BMH_ALIGNER_HOST_FORMAT")
    # strictly more than the exact mode flags, no more than marking alone
    exact = run(barcode_tag="RX", batch_reads=256)
    assert "pair_barcodes_observed" not in al.markdup_counts
    plain = run(batch_reads=256)
    assert _flagged(BamFile(exact[0]).stream) < _flagged(stream) <= _flagged(BamFile(plain[0]).stream)
    assert run(barcode_tag="RX", barcode_edits=0, batch_reads=256) == exact
    # refused before anything is written
    out = io.BytesIO()
    with pytest.raises(ValueError, match="barcode_tag or barcode_name"):
        al.align_files(path, out=out, paired=True, fmt="bam", sort=True, markdup=True, barcode_edits=1)
    with pytest.raises(ValueError, match="markdup"):
        al.align_files(path, out=out, paired=True, fmt="bam", sort=True, barcode_tag="RX", barcode_edits=1)
    with pytest.raises(ValueError, match="0 .. 21"):
        al.align_files(path, out=out, paired=True, fmt="bam", sort=True, markdup=True, barcode_tag="RX", barcode_edits=22)
    assert out.getvalue() == b""
    # edits without marking cannot be written down in the options record any more: the keywords refuse them, and the aligner stays as it was
    with pytest.raises(ValueError, match="marked"):
        al._native_aligner().set_sorted(barcode_edits=1)
    assert run(batch_reads=256) == plain
    al.close()


@pytest.mark.gpu
def test_mem_command(hip, tmp_path):
    path, names = _edited_reads(tmp_path)
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(common.GOLDEN), "..", "bwa-mem_gpu_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def mem(*args):
        return subprocess.run([sys.executable, "-m", "bwamem_hip.mem", *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    bam, met = str(tmp_path / "x.bam"), str(tmp_path / "m.txt")
    r = mem("-p", "-C", "--sort", "--markdup", "--markdup-metrics", met, "--barcode-tag", "RX", "--barcode-edits", "1", PREFIX, path, "-o", bam)
    assert r.returncode == 0, r.stderr.decode()
    with open(bam, "rb") as f:
        stream = _writer_order(BamFile(f.read()).stream, names)
    assert _flagged(stream) == _flagged(edits_model(stream, 1, tag="RX")[0]) and _flagged(stream)
    with open(met) as f:
        assert f.read().split("\n")[1].split("\t")[-2:] == ["READ_PAIR_DUPLICATES", "PERCENT_DUPLICATION"]      # the table keeps its columns
    for args, word in ((("-p", "-C", "--sort", "--markdup", "--barcode-edits", "1"), "--barcode-tag or --barcode-name"),
                       (("-p", "-C", "--sort", "--barcode-tag", "RX", "--barcode-edits", "1"), "--markdup"),
                       (("-p", "-C", "--sort", "--markdup", "--barcode-tag", "RX", "--barcode-edits", "22"), "0 .. 21")):
        r = mem(*args, PREFIX, path, "-o", str(tmp_path / "refused.bam"))
        assert r.returncode == 2 and word in r.stderr.decode() and not os.path.exists(str(tmp_path / "refused.bam"))
