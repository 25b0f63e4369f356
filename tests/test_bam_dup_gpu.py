"""Duplicate marking on the device: the corpus of test_bam_dup.py through the kernels (device bytes and counts equal the host forms'), the sorted file at every
window, reads -> marked sorted BAM end to end against the model of test_bam_dup.py applied to the output grouped by read name, across batch cuts, lane counts,
windows and a spilled run store, the ALT index, and the `python -m bwamem_hip.mem --sort --markdup` command."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import common
from test_bam_dup import DUP, corpus, expected, flag_of, mask_dup, model, name_of
from test_bam_gpu import PREFIX, _reads_files
from test_bam_sort import BamFile, check_file, split_records

HD = "@HD\tVN:1.6\tSO:coordinate\n"


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.mark.gpu
def test_device_equals_host(hip):
    """0 and 1 templates, 63 / 64 / 65 (wave edge), 257 (workgroup edge), 1000, and the 300 pairs at one key, whose run of equal lanes crosses a workgroup boundary"""
    from bwamem_hip.lib import bam_markdup
    for what, _contigs, stream, _must in corpus():
        want, counts, _h = expected(what, stream)
        got, c = bam_markdup(stream)
        assert (got, c) == bam_markdup(stream, host=True), what
        assert got == want and c == counts, what
    with pytest.raises(ValueError):
        bam_markdup(corpus()[0][2][:-1])


@pytest.mark.gpu
@pytest.mark.parametrize("window", [0, 1, 7, 100])
def test_sorted_file_device_equals_host(hip, window):
    from bwamem_hip.lib import bam_sorted_file
    for what, contigs, stream, _must in corpus():
        assert bam_sorted_file("@CO\tx\n", contigs, stream, 1, window, markdup=True) == bam_sorted_file("@CO\tx\n", contigs, stream, 1, window, host=True, markdup=True), (what, window)


# ---------------------------------------------------------------------------------------------------------------- end to end

def _dup_reads(tmp_path, paired, src=None):
    """the reads of _reads_files (or of the FASTA `src`) as FASTQ in which every fifth template appears three times under distinct names with different qualities,
    the copies behind all the originals (other batches); paired: read 2 of templates 5 and 35 is random (a fragment with an unmapped mate).  Returns (path, names
    in input order)"""
    path = src or _reads_files(tmp_path, paired)
    lines = open(path, "rb").read().split(b"\n")
    step = 4 if lines[0].startswith(b"@") else 2
    reads = [(lines[i][1:].split()[0], lines[i + 1]) for i in range(0, len(lines) - 1, step) if lines[i]]
    per = 2 if paired else 1
    tpls = [reads[i:i + per] for i in range(0, len(reads), per)]
    rng = np.random.default_rng(8)
    if paired:
        for t in (5, 35):
            tpls[t][1] = (tpls[t][1][0], bytes(rng.choice(list(b"ACGT"), len(tpls[t][1][1])).astype(np.uint8)))
    out, names = [], []
    for copy in range(3):
        for t, tp in enumerate(tpls):
            if copy and t % 5:
                continue
            for name, seq in tp:
                base, _, mate = name.partition(b"/")
                nm = base + (b"c%d" % copy if copy else b"")
                if not names or names[-1] != nm:
                    names.append(nm)
                q = bytes((rng.integers(2, 41, len(seq)) + 33).astype(np.uint8))
                out.append(b"@" + nm + (b"/" + mate if mate else b"") + b"\n" + seq + b"\n+\n" + q + b"\n")
    dst = str(tmp_path / "dups.fq")
    with open(dst, "wb") as f:
        f.write(b"".join(out))
    return dst, names


def _writer_order(stream: bytes, names) -> bytes:
    """the records of a sorted file back in the writer's order: by read name in input order, read 1 before read 2, the primary line first"""
    by = {}
    for i, r in enumerate(split_records(stream)):
        by.setdefault(name_of(r), []).append((bool(flag_of(r) & 0x80), bool(flag_of(r) & 0x900), i, r))
    assert set(by) == set(names)
    return b"".join(r for n in names for _a, _b, _i, r in sorted(by[n]))


def _run(al, path, markdup=True, **kw):
    out, idx = io.BytesIO(), io.BytesIO()
    al.align_file(path, out, fmt="bam", sort=True, index=idx, markdup=markdup, **kw)
    return out.getvalue(), idx.getvalue()


def _flagged(stream: bytes) -> set:
    return {name_of(r) for r in split_records(stream) if flag_of(r) & DUP}


def _check_marked(al, path, names, monkeypatch, tmp_path, **kw):
    paired = bool(kw.get("paired"))
    monkeypatch.setenv("BMH_ALIGNER_LANES", "1")
    bam, bai = _run(al, path, sort_window=100, batch_reads=256, **kw)
    assert al.last_stats.n_batches >= 3
    counts = dict(al.markdup_counts)
    plain, plain_bai = _run(al, path, markdup=False, sort_window=100, batch_reads=256, **kw)
    f, g = BamFile(bam), BamFile(plain)
    assert mask_dup(f.stream) == g.stream and not _flagged(g.stream)
    check_file(bam, bai, HD + al.header(), al.contigs, _writer_order(f.stream, names), "marked", n_regions=10)
    want, wc, _h = model(_writer_order(g.stream, names))
    assert {(name_of(r), flag_of(r)) for r in split_records(f.stream) if flag_of(r) & DUP} == {(name_of(r), flag_of(r)) for r in split_records(want) if flag_of(r) & DUP}
    assert counts == wc
    assert wc["duplicate_fragments"] >= 1 and (not paired or wc["duplicate_pairs"] >= 1)
    assert any(flag_of(r) & DUP and flag_of(r) & 0x900 for r in split_records(want))
    assert any(not flag_of(r) & DUP and not flag_of(r) & 4 for r in split_records(want))
    # where the batches are cut, how many lanes run, the window and a run store that spills every run do not change which templates are duplicates
    spill = tmp_path / "spill"; spill.mkdir()
    monkeypatch.setenv("BMH_ALIGNER_LANES", "2")
    for knobs in (dict(batch_reads=128, sort_window=7), dict(chunk_bases=30_000), dict(batch_reads=256, sort_window=100, sort_mem=1, sort_tmp=str(spill))):
        b2, _i2 = _run(al, path, **knobs, **kw)
        assert al.last_stats.n_batches >= 3
        assert _flagged(BamFile(b2).stream) == _flagged(f.stream), knobs
    assert os.listdir(spill) == []
    monkeypatch.setenv("BMH_ALIGNER_HOST_FORMAT", "1")                 # batches the host formats go through the host forms of the entries
    assert BamFile(_run(al, path, sort_window=100, batch_reads=256, **kw)[0]).stream == f.stream
    monkeypatch.delenv("BMH_ALIGNER_HOST_FORMAT")
    assert _run(al, path, markdup=False, sort_window=100, batch_reads=256, **kw) == (plain, plain_bai)        # the option is switched off again


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_reads_to_marked_sorted_bam(hip, tmp_path, monkeypatch, paired):
    from bwamem_hip.aligner import Aligner
    path, names = _dup_reads(tmp_path, paired)
    al = Aligner(PREFIX, n_threads=4)
    _check_marked(al, path, names, monkeypatch, tmp_path, paired=paired)
    al.close()


@pytest.mark.gpu
def test_reads_to_marked_sorted_bam_alt_index(hip, tmp_path, monkeypatch):
    """several contigs, ALT contigs among them (the genome and reads of tests/golden/alt_golden.npz)"""
    import ast
    from bwamem_hip import fmindex, synth
    from bwamem_hip.aligner import Aligner
    z = np.load(os.path.join(common.GOLDEN, "alt_golden.npz"))
    n = int(z["n_genome"]); bits = np.unpackbits(z["genome_packed"])[: 2 * n].reshape(n, 2)
    g = (bits[:, 0] * 2 + bits[:, 1]).astype(np.uint8)
    prefix = str(tmp_path / "g.fa")
    fmindex.write_index(prefix, fmindex.build_fmd_index(g)); fmindex.write_bns(prefix, g, contigs=ast.literal_eval(str(z["contigs"])))
    with open(prefix + ".alt", "wb") as f:
        f.write(bytes(z["alt_file"]))
    asc = synth.codes_to_ascii(z["reads"])
    src = str(tmp_path / "r.fa")
    with open(src, "wb") as f:
        for i in range(len(asc)):
            f.write(b">r%d\n%s\n" % (i, asc[i].tobytes()))
    path, names = _dup_reads(tmp_path, False, src)
    al = Aligner(prefix, n_threads=4)
    assert al.has_alt and len(al.contigs) > 1
    monkeypatch.setenv("BMH_ALIGNER_LANES", "2")
    out, idx = io.BytesIO(), io.BytesIO()
    al.align_file(path, out, fmt="bam", sort=True, index=idx, markdup=True, sort_window=100, batch_reads=256)
    plain = io.BytesIO(); al.align_file(path, plain, fmt="bam", sort=True, sort_window=100, batch_reads=256)
    f, p = BamFile(out.getvalue()), BamFile(plain.getvalue())
    assert mask_dup(f.stream) == p.stream
    check_file(out.getvalue(), idx.getvalue(), HD + al.header(), al.contigs, _writer_order(f.stream, names), "ALT", n_regions=10)
    want, wc, _h = model(_writer_order(p.stream, names))
    assert _writer_order(f.stream, names) == want and al.markdup_counts == wc and wc["duplicate_fragments"] >= 1
    assert any(flag_of(r) & DUP and flag_of(r) & 0x900 for r in split_records(want)) and any(not flag_of(r) & DUP and not flag_of(r) & 4 for r in split_records(want))
    al.close()


@pytest.mark.gpu
def test_mem_command_markdup(hip, tmp_path):
    from bwamem_hip.aligner import Aligner
    path, _names = _dup_reads(tmp_path, True)
    env = dict(os.environ, PYTHONPATH=os.path.join(os.path.dirname(common.GOLDEN), "..", "bwa-mem_gpu_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def mem(*args):
        return subprocess.run([sys.executable, "-m", "bwamem_hip.mem", *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    bam, met = str(tmp_path / "x.bam"), str(tmp_path / "m.txt")
    r = mem("-p", "-R", "@RG\\tID:g\\tLB:lib1\\tSM:s", "--sort", "--markdup", "--markdup-metrics", met, PREFIX, path, "-o", bam)
    assert r.returncode == 0, r.stderr.decode()
    al = Aligner(PREFIX)
    al.set_options(["-R", "@RG\\tID:g\\tLB:lib1\\tSM:s"])
    out, idx = io.BytesIO(), io.BytesIO()
    al.align_file(path, out, paired=True, fmt="bam", sort=True, index=idx, markdup=True)      # the same reads and options in this process
    c = al.markdup_counts
    al.close()
    with open(bam, "rb") as f, open(bam + ".bai", "rb") as g:
        assert f.read() == out.getvalue() and g.read() == idx.getvalue()
    lines = open(met).read().split("\n")
    assert lines[0].startswith("## METRICS CLASS")
    row = dict(zip(lines[1].split("\t"), lines[2].split("\t")))
    assert row["LIBRARY"] == "lib1" and c["duplicate_pairs"] >= 1
    assert [int(row[k]) for k in ("UNPAIRED_READS_EXAMINED", "READ_PAIRS_EXAMINED", "SECONDARY_OR_SUPPLEMENTARY_RDS", "UNMAPPED_READS", "UNPAIRED_READ_DUPLICATES", "READ_PAIR_DUPLICATES")] == \
        [c[k] for k in ("fragments_examined", "pairs_examined", "secondary_or_supplementary", "unmapped_records", "duplicate_fragments", "duplicate_pairs")]
    assert abs(float(row["PERCENT_DUPLICATION"]) - (c["duplicate_fragments"] + 2 * c["duplicate_pairs"]) / (c["fragments_examined"] + 2 * c["pairs_examined"])) < 1e-5
    assert mem("--markdup", PREFIX, path).returncode == 2
