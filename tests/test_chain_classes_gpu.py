"""Every size class, lane bin and contig-table form of the device chaining kernels (csrc/chain_kernels.hip) at its limits: the reads of
tests/chain_classes.py sample 2 .. 2002 seed occurrences, exactly at and one beyond every boundary of chain_classify_kernel.  Each case is the full
device case of tests/chain_case.py -- bmh_chain_batch byte for byte against the host job builder, extension and merge against the oracle, the form
without materialised bases and the one-call form -- and in addition pins WHICH form chained each read: ChainWorkspace.class_counts() equals the
classification restated on the host, and every class or bin the case is about holds reads.  (The same reads through the serial CPU build of the
chaining core: tests/test_host_jobs.py.)"""
import hashlib
import time

import numpy as np
import pytest

import chain_classes as cc
from chain_case import _device_chain_case

pytestmark = pytest.mark.gpu

CLASSES = tuple(range(cc.N_CLASSES))                       # indices into class_counts(): the size classes ...
BINS = tuple(range(cc.N_CLASSES, cc.N_CLASSES + 4))        # ... the lane kernel's bins (the fourth: beyond 8 entries, up to the lane threshold) ...
LONG = 15                                                  # ... the reads of the long-read kernel


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()           # raises if the HIP extension is missing: no fallback
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


class _SharedOracle:
    """the oracle's extension, computed once per distinct job batch (most cases build the same jobs by different kernels) and never written to"""

    def __init__(self, oracle):
        self.oracle, self.memo = oracle, {}

    def extend_batch(self, q, qoff, qlen, t, toff, tlen, h0, params=None):
        key = hashlib.sha1(b"".join(np.ascontiguousarray(x).tobytes() for x in (q, qoff, qlen, t, toff, tlen, h0)) + bytes(params)).digest()
        if key not in self.memo:
            out3, _, cells = self.oracle.extend_batch(q, qoff, qlen, t, toff, tlen, h0, params=params, n_threads=4)
            out3.setflags(write=False)
            self.memo[key] = (out3, None, cells)
        return self.memo[key]


@pytest.fixture(scope="module")
def orc(oracle):
    return _SharedOracle(oracle)


def _long_reads():
    """two reads beyond CH_MAX_READ_LEN (720 bases of the genome's random tail, two mismatches; one reversed): the long-read kernel"""
    from bwamem_hip import synth
    g = cc.genome()[0]
    x = g[len(g) - 30_000: len(g) - 30_000 + 720].copy()
    x[[200, 500]] = (x[[200, 500]] + 1) & 3
    return [x, synth.revcomp(x)]


def _case(hip, orc, name, must, rows=None, heavy=None, opt_over=None, **kw):
    """must: {index into class_counts(): fewest reads the case needs there}"""
    g, idx = cc.genome()[:2]
    rows = cc.reads() if rows is None else rows
    max_occ = (opt_over or {}).get("max_occ", 500)
    seen = []

    def on_counts(seeds, lens, counts):
        need, where, want = cc.classify(seeds, lens, max_occ, cc.DEFAULT_HEAVY if heavy is None else heavy)
        if not seen:
            print(f"\nchain classes [{name}]: class_counts {counts.tolist()}  largest need {int(need.max())}")
        assert np.array_equal(counts, want), (counts.tolist(), want.tolist())
        assert int(want.sum()) == len(lens)                  # every read in exactly one form
        short = {k: int(want[k]) for k, m in must.items() if want[k] < m}
        assert not short, f"the case is about forms that hold too few reads: {short}"
        seen.append(counts)
    t0 = time.time()
    nj, nr, nh = _device_chain_case(hip, orc, g, idx, rows, opt_over=opt_over, heavy=heavy, on_counts=on_counts, **kw)
    print(f"chain classes [{name}]: {len(rows)} reads, {nj} jobs, {nr} regions, {time.time() - t0:.2f} s")
    assert len(seen) == 3 and nh == int(seen[0][:cc.N_CLASSES].sum())
    return seen[0]


def at_least(idx, m=2):
    return {k: m for k in idx}


def test_default_options_every_class_every_bin_and_long_reads(hip, orc):
    """default options: all eleven classes, the three bins a threshold of 8 leaves, the long-read kernel; more located than sampled (700 copies)"""
    _case(hip, orc, "default", at_least(CLASSES + BINS[:3] + (LONG,)), rows=cc.reads() + _long_reads())


@pytest.mark.parametrize("grid_max,reverse", [(1, False), (2, True)])
def test_blocks_chain_read_after_read_through_one_scratch(hip, orc, grid_max, reverse):
    """CHAIN_GRID_MAX: one or two blocks per class, six reads or more in each -- a block chains a large read, then a small one through the same LDS slice
    (or the reverse: the reads in the opposite order); what a read leaves in the scratch must not reach the next"""
    _case(hip, orc, f"grid_max={grid_max}", at_least(CLASSES, 6), rows=cc.reads(repeat=2, reverse=reverse), grid_max=grid_max)


@pytest.mark.parametrize("over,must", [(dict(max_occ=50), CLASSES[:5] + BINS[:3]), (dict(max_occ=7, max_chain_extend=3), (2, 3) + BINS[:3])], ids=["c50", "c7_x3"])
def test_more_located_than_sampled(hip, orc, over, must):
    """a small max_occ: reads sample few of many located seeds -- the four-per-wave classes stage the located ones, so the classification moves such a read
    by that count (to class 3 at most); the lane kernel's private arrays hold the sampled ones only"""
    c = _case(hip, orc, "max_occ=%d" % over["max_occ"], at_least(must), opt_over=over)
    assert c[3] >= 20                                        # (need <= 64 < located: moved to the first wave class)


@pytest.mark.parametrize("heavy", [None, 0])
def test_seed_filter_forms(hip, orc, heavy):
    """min_chain_weight 3: the reference's seed filter applies from 66 bases on (the reads of several units), so every kernel runs in its form with the
    filter compiled in and WIDE scratch records -- the hybrid classes then keep klist and cidx in global memory too"""
    _case(hip, orc, f"W=3 heavy={heavy}", at_least(CLASSES + (BINS[:3] if heavy is None else ())), opt_over=dict(min_chain_weight=3), heavy=heavy)


@pytest.mark.parametrize("sub", [7, 0, 5])
def test_every_read_by_a_cooperative_form(hip, orc, sub):
    """lane threshold 0: the reads of 2 .. 8 entries join class 0; CHAIN_SUB: classes 0-2 four reads per wave (7), a lane or a wave per read (0), mixed (5)"""
    _case(hip, orc, f"heavy=0 sub={sub}", at_least(CLASSES), heavy=0, sub=sub)


@pytest.mark.parametrize("heavy,empty", [(12, ()), (16, (0,)), (40, (0, 1))])
def test_lane_kernel_private_scratch_sizes(hip, orc, heavy, empty):
    """lane thresholds 12, 16, 40: private scratch of 12 and 16 entries and the global slices, with reads exactly at the threshold (the lane kernel's fourth
    bin) and one beyond it (the first class that is left)"""
    _case(hip, orc, f"heavy={heavy}", at_least(tuple(c for c in CLASSES if c not in empty) + BINS), heavy=heavy)


@pytest.mark.parametrize("heavy", [None, 0])
@pytest.mark.parametrize("n_contigs", [3, 100, 300])
def test_contig_table_forms(hip, orc, n_contigs, heavy):
    """3, 100 and 300 sequences over the same genome, cut inside spacers and through unit copies: the contig table's copy in LDS of 64 entries (wave and
    four-per-wave kernels), of 256 (wave kernels; the four-per-wave ones read global memory) and none"""
    _case(hip, orc, f"contigs={n_contigs} heavy={heavy}", at_least(CLASSES + (BINS[:3] if heavy is None else ())), heavy=heavy, contigs=cc.contig_table(n_contigs))
