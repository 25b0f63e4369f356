"""The life of the host-side device memory (csrc/devmem.h) under the whole aligner: the lanes' grow-only buffers and the per-(device, stream) scratch of the
extension, the region tail, the mate rescue and the CIGAR stage grow after their first use, are used again at a smaller size, are released with their streams
and made again in the same process -- and the SAM text never changes.  The registry and the growth rule alone: tests/test_devmem.py."""
import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

CUTS = [0, 64, 64 + 4096, 64 + 4096 + 64]          # a small batch, one that makes every buffer grow, a small one in the grown buffers


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip
    bwamem_hip.load_library()
    assert torch.cuda.is_available(), "this test needs a GPU"
    return bwamem_hip


def _run(al, rs, cuts):
    """the batches of `cuts` in one native run on ONE lane (one stream, one set of buffers, batch after batch): the text of every batch"""
    parts = []
    al._native_aligner().run(rs, cuts, True, lambda mv: parts.append(bytes(mv)), n_lanes=1, n_threads=2)
    assert len(parts) == len(cuts) - 1
    return parts


def test_scratch_grows_is_reused_released_and_recreated(hip, tmp_path):
    from bwamem_hip import fmindex, synth
    from bwamem_hip.aligner import Aligner, read_fasta_reads
    g, idx = common.genome_and_index(300_000)
    prefix = str(tmp_path / "g.fa")
    fmindex.write_index(prefix, idx); fmindex.write_bns(prefix, g)
    asc = synth.codes_to_ascii(synth.make_pairs(g, CUTS[-1] // 2, 150, seed=31, sub_rate=0.02)[0])
    fq = str(tmp_path / "r.fa")
    with open(fq, "wb") as f:
        for i in range(len(asc)):
            f.write(b">p%d\n" % (i // 2)); f.write(asc[i].tobytes()); f.write(b"\n")
    rs = read_fasta_reads(fq)
    assert len(rs) == CUTS[-1]
    # the reference: every batch alone, each by an aligner that has done nothing else (id0: the index of the batch's first read in the run, which the tie-break
    # hash takes -- a native run numbers its reads from 0, so the batch alone goes through align_batch, which writes the same text: test_gpu_parity.py)
    want = []
    for b, e in zip(CUTS[:-1], CUTS[1:]):
        fresh = Aligner(prefix, n_threads=2)
        want.append(bytes(fresh.align_batch(rs.slice(b, e), id0=b, paired=True, as_bytes=True)))
        fresh.close()
    assert all(w.count(b"\n") >= e - b for w, b, e in zip(want, CUTS[:-1], CUTS[1:])) and len(set(want)) == 3
    # one aligner, one lane: 64 reads, 4096 reads (growth after first use), 64 reads (the grown buffers)
    al = Aligner(prefix, n_threads=2)
    got = _run(al, rs, CUTS)
    for k in range(3):
        assert got[k] == want[k], ("native run, batch", k, _first_diff(got[k], want[k]))
    # the same three through the batch-after-batch loop: the stages' scratch of the stream PyTorch runs on grows and is used again likewise
    for k, (b, e) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        txt = al.align_batch(rs.slice(b, e), id0=b, paired=True, as_bytes=True)
        assert bytes(txt) == want[k], ("batch loop, batch", k, _first_diff(bytes(txt), want[k]))
    al.close()
    # released; a second aligner in the same process (new lanes, recycled stream handles) and the first batch again
    al2 = Aligner(prefix, n_threads=2)
    again = _run(al2, rs.slice(0, CUTS[1]), CUTS[:2])
    assert again[0] == want[0], ("second aligner", _first_diff(again[0], want[0]))
    al2.close()


def _first_diff(a: bytes, b: bytes):
    la, lb = a.split(b"\n"), b.split(b"\n")
    return len(la), len(lb), [(x, y) for x, y in zip(la, lb) if x != y][:1]
