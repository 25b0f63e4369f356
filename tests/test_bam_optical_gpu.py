"""Optical duplicates on the device: the locations and counts of test_bam_optical.py's corpus through the kernels (equal to the host forms'), sets built for the
clustering's edges -- chains across wave, workgroup and grid-block boundaries, long walks without a union, thousands of small sets, a set across the compacted
array's 256-lane boundary, three libraries -- and reads -> marked sorted BAM end to end through align_files, align_groups and keep_rg: the counts equal the model
of test_bam_optical.py applied to the output grouped by read name, they do not change with batch cuts or a spilling run store, and the file is byte for byte that of
the run without the option."""
import io
import os

import numpy as np
import pytest

from test_bam_dup_gpu import _writer_order
from test_bam_gpu import PREFIX, _reads_files
from test_bam_optical import CORPUS_KW, GROUPS, assert_equals_model, cases, model_counts, nm, opair, random_corpus
from test_bam_sort import CONTIGS, BamFile, py_sort

OPT = ("optical_duplicate_pairs", "located_pairs", "optical_sets_skipped")


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
    return got[1]


@pytest.mark.gpu
def test_device_equals_host_on_the_corpus(hip):
    from bwamem_hip.lib import bam_dup_locations, bam_markdup
    members = [(c[0], c[1], c[2]) for c in cases()] + [("corpus", random_corpus(), CORPUS_KW), ("corpus, default max_set", random_corpus(), dict(CORPUS_KW, optical_max_set=None))]
    for what, stream, kw in members:
        counts = _both(stream, **kw)
        assert_equals_model(counts, stream, kw, what)
        groups = kw.get("read_groups")
        L = bam_dup_locations(stream, read_groups=groups)
        assert L.tobytes() == bam_dup_locations(stream, host=True, read_groups=groups).tobytes(), what
        base = {k: v for k, v in kw.items() if not k.startswith("optical")}
        assert bam_markdup(stream, **kw)[0] == bam_markdup(stream, **base)[0], what
    assert len(bam_dup_locations(random_corpus())) > 400          # (without read groups: no tag is read)


def _flat(tpls):
    return b"".join(r for t in tpls for r in t)


@pytest.mark.gpu
def test_chains(hip):
    """chains of touching members -- neighbours exactly D apart, so every union is needed -- of lengths around a wave, a workgroup and several workgroups; the
    members come in shuffled order, half of the chains run along y"""
    D = 7
    rng = np.random.default_rng(2)
    tpls, want = [], 0
    for c, n in enumerate((63, 64, 65, 255, 256, 257, 1025)):
        for i in range(n):
            x, y = (500, 10 + i * D) if c & 1 else (10 + i * D, 500)
            tpls.append(opair(nm(3, x, y, k=len(tpls)), 1000 + 100 * c, 5000 + 100 * c))
        want += n - 1
    order = rng.permutation(len(tpls))
    counts = _both(_flat([tpls[i] for i in order]), optical_distance=D)
    assert [counts[k] for k in OPT] == [want, len(tpls), 0] and counts["duplicate_pairs"] == want
    # one pixel less and every chain falls apart
    assert _both(_flat([tpls[i] for i in order]), optical_distance=D - 1)["optical_duplicate_pairs"] == 0
    # the largest set alone is skipped at max_set 1024, and taken at 1025
    assert [_both(_flat(tpls), optical_distance=D, optical_max_set=m)[k] for m in (1024, 1025) for k in ("optical_duplicate_pairs", "optical_sets_skipped")] == [want - 1024, 1, want, 0]


@pytest.mark.gpu
def test_long_walks_without_a_union(hip):
    """600 pairs of one set at one x, their ys 2 D apart: every lane walks to the end of the set and unites nothing"""
    D = 50
    tpls = [opair(nm(1, 777, i * 2 * D, k=i), 100, 300) for i in range(600)]
    counts = _both(_flat(tpls), optical_distance=D)
    assert [counts[k] for k in OPT] == [0, 600, 0] and counts["duplicate_pairs"] == 599
    # ... and with ys D apart, one cluster
    tpls = [opair(nm(1, 777, i * D, k=i), 100, 300) for i in range(600)]
    assert _both(_flat(tpls), optical_distance=D)["optical_duplicate_pairs"] == 599


@pytest.mark.gpu
def test_many_small_sets(hip):
    """3000 sets of 2 across the grid's blocks: every other one a cluster"""
    tpls = []
    for s in range(3000):
        tpls.append(opair(nm(1 + s % 3, 100, 100, k=2 * s), 1000 + 3 * s, 20000 + 3 * s))
        tpls.append(opair(nm(1 + s % 3, 100 + (10 if s & 1 else 11), 100, k=2 * s + 1), 1000 + 3 * s, 20000 + 3 * s))
    order = np.random.default_rng(4).permutation(len(tpls))
    counts = _both(_flat([tpls[i] for i in order]), optical_distance=10)
    assert [counts[k] for k in OPT] == [1500, 6000, 0] and counts["duplicate_pairs"] == 3000


@pytest.mark.gpu
def test_a_set_across_the_compacted_arrays_boundary(hip):
    """127 sets of 2 fill the members' places 0 .. 253; the next set, a chain of 5, takes 254 .. 258 -- across the 256-lane boundary; unlocated pairs and sets of
    one in between shift the templates' places against the members'"""
    D = 5
    tpls = []
    for s in range(127):
        tpls += [opair(nm(1, 10, 10, k=len(tpls)), 1000 + 5 * s, 9000), opair(b"unlocated%d" % s, 1000 + 5 * s, 9000), opair(nm(1, 10, 16, k=len(tpls) + 1), 1000 + 5 * s, 9000),
                 opair(nm(1, 10, 10, k=len(tpls) + 2), 1002 + 5 * s, 9000)]
    tpls += [opair(nm(2, 100 + D * i, 100, k=len(tpls) + i), 3000, 9000) for i in range(5)]
    tpls += [opair(nm(2, 100, 100, k=len(tpls) + i), 3100, 9000) for i in range(2)]
    stream = _flat(tpls)
    counts = _both(stream, optical_distance=D)
    assert [counts[k] for k in OPT] == [4 + 1, 127 * 3 + 5 + 2, 0]
    assert_equals_model(counts, stream, dict(optical_distance=D), "boundary")


@pytest.mark.gpu
def test_three_libraries(hip):
    groups = [(b"g0", "L0"), (b"g1", "L1"), (b"g2", "L2"), (b"g3", "L1")]
    tpls = []
    for s in range(300):
        g = groups[s % 4][0]
        n = 2 + s % 3
        tpls += [opair(nm(1, 50 + 3 * i, 50, k=len(tpls) + i), 1000 + 7 * (s // 4), 30000, rg=g) for i in range(n)]       # the same keys in every library
    stream = _flat(tpls)
    kw = dict(optical_distance=3, read_groups=groups)
    counts = _both(stream, **kw)
    assert_equals_model(counts, stream, kw, "three libraries")
    per = {lb: c["optical_duplicate_pairs"] for lb, c in counts["libraries"].items()}
    assert list(per) == ["L0", "L1", "L2"] and all(v > 0 for v in per.values()) and sum(per.values()) == counts["optical_duplicate_pairs"]


@pytest.mark.gpu
def test_sorted_file_bytes_unchanged(hip):
    from bwamem_hip.lib import bam_markdup, bam_sorted_file
    stream = random_corpus()
    marked, counts = bam_markdup(stream, **CORPUS_KW)
    bam, bai, c2 = bam_sorted_file("@CO\tx\n", CONTIGS, stream, 1, 100, markdup=True, read_groups=GROUPS)
    assert (bam, bai, c2) == bam_sorted_file("@CO\tx\n", CONTIGS, stream, 1, 100, host=True, markdup=True, read_groups=GROUPS)
    assert BamFile(bam).stream == py_sort(marked) and all(counts[k] == v for k, v in c2.items() if k != "libraries")


# ---------------------------------------------------------------------------------------------------------------- end to end

D_E2E = 100
IDS = ["a", "ab", "lane.3-of_three"]
LINES = ["@RG\tID:a\tLB:libX\tSM:s", "@RG\tID:ab\tSM:s\tLB:libX\tPU:unit.2", "@RG\tID:lane.3-of_three\tLB:libY\tSM:s"]
TABLE = [(b"a", "libX"), (b"ab", "libX"), (b"lane.3-of_three", "libY")]


def _optical_reads(tmp_path):
    """_reads_files' 300 pairs as FASTQ under Illumina-style names (seven fields); every fifth pair has three copies behind all the originals (other batches):
    one D to the right, one another D to the right and D up (a chain of three), one far away.  Returns (path, names in input order, {name: group}) -- the groups
    for the runs over read groups: the chain of every tenth pair lies in one lane of library Y, of the others' the last member lies in library X's other lane"""
    src = _reads_files(tmp_path, True)
    lines = open(src, "rb").read().split(b"\n")
    reads = [(lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4) if lines[i]]
    out, names, group = [], [], {}
    for copy in range(4):
        for t in range(len(reads) // 2):
            if copy and t % 5 != 1:                              # (not the chimeric and random reads: those are every fifth pair from 0)
                continue
            x0, y0 = 1000 + 11 * t, 2000 + 7 * t
            x, y = [(x0, y0), (x0 + D_E2E, y0), (x0 + 2 * D_E2E, y0 + D_E2E), (x0 + 50_000, y0)][copy]
            name = b"M01:%d:FC:1:%d:%d:%d" % (7 + copy, 1101 + t % 3, x, y)
            names.append(name)
            group[name] = "lane.3-of_three" if t % 10 == 6 else ("ab" if copy == 2 else "a") if t % 5 == 1 else IDS[t % 3]
            for m in (0, 1):
                seq, q = reads[2 * t + m]
                out.append(b"@" + name + b"/%d\n" % (m + 1) + seq + b"\n+\n" + q + b"\n")
    path = str(tmp_path / "optical.fq")
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return path, names, group


def _metrics_rows(text):
    lines = text.split("\n")
    assert lines[0].startswith("## METRICS CLASS") and lines[-1] == ""
    assert lines[1].split("\t")[-4:] == ["READ_PAIR_DUPLICATES", "READ_PAIR_OPTICAL_DUPLICATES", "PERCENT_DUPLICATION", "ESTIMATED_LIBRARY_SIZE"]
    return {r.split("\t")[0]: dict(zip(lines[1].split("\t"), r.split("\t"))) for r in lines[2:-1]}


def _check_row(row, c):
    from bwamem_hip.lib import estimate_library_size
    assert [int(row[k]) for k in ("READ_PAIRS_EXAMINED", "READ_PAIR_DUPLICATES", "READ_PAIR_OPTICAL_DUPLICATES", "UNPAIRED_READS_EXAMINED")] == \
        [c[k] for k in ("pairs_examined", "duplicate_pairs", "optical_duplicate_pairs", "fragments_examined")]
    size = estimate_library_size(c["pairs_examined"] - c["optical_duplicate_pairs"], c["pairs_examined"] - c["duplicate_pairs"])
    assert row["ESTIMATED_LIBRARY_SIZE"] == ("" if size is None else str(size)) and size is not None


@pytest.mark.gpu
def test_reads_to_optical_counts(hip, tmp_path, monkeypatch):
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.lib import bam_markdup
    path, names, _group = _optical_reads(tmp_path)
    al = Aligner(PREFIX, n_threads=4)
    monkeypatch.setenv("BMH_ALIGNER_LANES", "2")

    def run(optical=True, **knobs):
        out, idx, met = io.BytesIO(), io.BytesIO(), io.StringIO()
        al.align_files(path, out=out, paired=True, fmt="bam", sort=True, index=idx, markdup=True, markdup_metrics=met, sort_window=100,
                       **(dict(optical_distance=D_E2E) if optical else {}), **knobs)
        assert al.last_stats.n_batches >= 3
        return out.getvalue(), idx.getvalue(), met.getvalue()
    spill = tmp_path / "spill"; spill.mkdir()
    base = run(batch_reads=256)
    counts, opt = dict(al.markdup_counts), dict(al.markdup_optical_counts)
    assert {k: counts[k] for k in OPT} == opt
    # the model, and the host form, on the output grouped by name
    stream = _writer_order(BamFile(base[0]).stream, names)
    total, _per, stats = model_counts(stream, dict(optical_distance=D_E2E))
    assert opt == total and total["optical_duplicate_pairs"] >= 80 and max(stats["sizes"]) == 3 and total["located_pairs"] == counts["pairs_examined"]
    assert total["optical_duplicate_pairs"] < counts["duplicate_pairs"]                 # the copies far away are duplicates and no optical ones
    assert bam_markdup(stream, host=True, optical_distance=D_E2E)[1] == counts
    _check_row(_metrics_rows(base[2])["Unknown Library"], counts)
    # batch cuts and a run store that spills every run: the same counts
    for knobs in (dict(batch_reads=128), dict(batch_reads=256, sort_mem=1, sort_tmp=str(spill))):
        run(**knobs)
        assert dict(al.markdup_optical_counts) == opt, knobs
    assert os.listdir(spill) == []
    # without the option: the same file and index, today's counts and table
    plain = run(optical=False, batch_reads=256)
    assert plain[:2] == base[:2] and "OPTICAL" not in plain[2] and not any(k in al.markdup_counts for k in OPT)
    assert al.markdup_counts == {k: v for k, v in counts.items() if k not in OPT}
    monkeypatch.setenv("BMH_ALIGNER_HOST_FORMAT", "1")                 # batches the host formats bring their locations through the host form
    assert run(batch_reads=256)[:2] == base[:2] and dict(al.markdup_optical_counts) == opt
    al.close()


def _split_by_group(tmp_path, path, group):
    """the FASTQ's records into one file per group, in input order"""
    lines = open(path, "rb").read().split(b"\n")
    files = {g: [] for g in IDS}
    for i in range(0, len(lines) - 1, 4):
        files[group[lines[i][1:].partition(b"/")[0]]].append(b"\n".join(lines[i:i + 4]) + b"\n")
    out = {}
    for g, recs in files.items():
        out[g] = str(tmp_path / ("group_%d.fq" % IDS.index(g)))
        with open(out[g], "wb") as f:
            f.write(b"".join(recs))
    return out


def _check_groups_run(al, out, met, names):
    stream = _writer_order(BamFile(out).stream, names)
    kw = dict(optical_distance=D_E2E, read_groups=TABLE)
    total, per, _stats = model_counts(stream, kw)
    assert dict(al.markdup_optical_counts) == total and al.markdup_library_optical_counts == per and list(per) == ["libX", "libY"]
    assert all(v["optical_duplicate_pairs"] >= 20 for v in per.values())
    # a copy in the library's other lane is a duplicate and no optical one: fewer than the run without groups counts
    assert total["optical_duplicate_pairs"] < model_counts(stream, dict(optical_distance=D_E2E))[0]["optical_duplicate_pairs"]
    rows = _metrics_rows(met)
    for lb in per:
        _check_row(rows[lb], al.markdup_library_counts[lb])


@pytest.mark.gpu
def test_groups_and_keep_rg(hip, tmp_path, monkeypatch):
    from bwamem_hip.aligner import Aligner
    from test_keep_rg_gpu import _fastx, _input_bam
    path, names, group = _optical_reads(tmp_path)
    al = Aligner(PREFIX, n_threads=4)
    monkeypatch.setenv("BMH_ALIGNER_LANES", "2")
    files = _split_by_group(tmp_path, path, group)
    kw = dict(fmt="bam", sort=True, markdup=True, sort_window=100, batch_reads=256)
    out, idx, met = io.BytesIO(), io.BytesIO(), io.StringIO()
    al.align_groups([(LINES[k], files[g], None) for k, g in enumerate(IDS)], out=out, paired=True, index=idx, markdup_metrics=met, optical_distance=D_E2E, **kw)
    _check_groups_run(al, out.getvalue(), met.getvalue(), names)
    plain, plain_idx = io.BytesIO(), io.BytesIO()
    al.align_groups([(LINES[k], files[g], None) for k, g in enumerate(IDS)], out=plain, paired=True, index=plain_idx, **kw)
    assert (plain.getvalue(), plain_idx.getvalue()) == (out.getvalue(), idx.getvalue())
    # the input's own read groups: one BAM whose records name them
    bam = _input_bam(tmp_path, "optical.bam", _fastx(path), True, lambda t: group[names[t]], LINES)
    out, idx, met = io.BytesIO(), io.BytesIO(), io.StringIO()
    al.align_files(bam, out=out, keep_rg=True, index=idx, markdup_metrics=met, optical_distance=D_E2E, **kw)
    _check_groups_run(al, out.getvalue(), met.getvalue(), names)
    plain, plain_idx = io.BytesIO(), io.BytesIO()
    al.align_files(bam, out=plain, keep_rg=True, index=plain_idx, **kw)
    assert (plain.getvalue(), plain_idx.getvalue()) == (out.getvalue(), idx.getvalue())
    al.close()
