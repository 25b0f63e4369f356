"""A genome and reads that land on both sides of every size-class and lane-bin boundary of the device job builder
(csrc/chain_kernels.hip: chain_classify_kernel), and that classification restated on the host.

Genome: families of a 50-base random unit, family i inserted FAMILIES[i] times as exact copies, all copies in shuffled order with unique
random spacers of 30-59 bases between them, then 50 kb of random sequence.  A read is one unit, or units of different families joined by a
single N (code 4): the N ends every supermaximal match at the unit's edge -- without it the match runs a few bases into the neighbouring unit
and its occurrence count collapses --, so a read's SMEMs are its units, unit i with FAMILIES[i] occurrences, and the number of occurrences the
chaining core samples for it is exactly sum(min(FAMILIES[i], max_occ)).  Every read comes with its reverse complement."""
from __future__ import annotations

import functools

import numpy as np

from bwamem_hip import fmindex, synth

UNIT = 50
# (3 and 5: one beyond the first two bins of the lane kernel; four families of 500 copies: the reads that sample 1250, 1860 and 2000 occurrences join up to four of them; 700: more located than sampled at max_occ = 500)
FAMILIES = (2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 384, 385, 500, 500, 500, 500, 512, 513, 700, 120, 121, 250, 251, 360, 361)
_F = {k: FAMILIES.index(k) for k in FAMILIES}          # family of a copy count (500: the first of the four)
_F500 = [i for i, k in enumerate(FAMILIES) if k == 500]
# reads of several units, as family indices; their need at max_occ = 500: 620, 621, 1250, 1251, 1860, 1861, 2000, 2002, 512, 513, 620 (700 capped at 500), and
# 40 / 41: the pair around a lane threshold of 40 (BMH_CHAIN_HEAVY)
COMBOS = ([_F500[0], _F[120]], [_F500[1], _F[121]], [_F500[0], _F500[1], _F[250]], [_F500[2], _F500[3], _F[251]], _F500[:3] + [_F[360]], _F500[1:] + [_F[361]],
          list(_F500), _F500 + [_F[2]], [_F500[2], _F[12]], [_F500[3], _F[13]], [_F[700], _F[120]], [_F[32], _F[8]], [_F[32], _F[9]])

N_BINS, N_CLASSES, N_SUB = 4, 11, 3
BIN_CAPS = (2, 4, 8)                                                    # ch_bin_of
CLASS_CAPS = (16, 32, 64, 128, 256, 384, 512, 620, 1250, 1860)          # ch_class_of; beyond the last: class 10
MAX_READ_LEN = 700                                                      # CH_MAX_READ_LEN: longer reads take chain_long_kernel
DEFAULT_HEAVY = 8                                                       # CH_HEAVY_DEFAULT


@functools.lru_cache(maxsize=1)
def genome():
    """(genome codes uint8, FMD index, start of every unit copy int64 [n_copies], family of every copy, the units)"""
    rng = np.random.default_rng(20250)
    units = [rng.integers(0, 4, size=UNIT).astype(np.uint8) for _ in FAMILIES]
    fam = np.repeat(np.arange(len(FAMILIES)), FAMILIES)
    rng.shuffle(fam)
    parts, starts, pos = [], np.zeros(len(fam), np.int64), 0
    for j, f in enumerate(fam):
        sp = rng.integers(0, 4, size=int(rng.integers(30, 60))).astype(np.uint8)
        parts += [sp, units[f]]
        starts[j] = pos + len(sp)
        pos += len(sp) + UNIT
    parts.append(rng.integers(0, 4, size=50_000).astype(np.uint8))
    g = np.concatenate(parts)
    return g, fmindex.build_fmd_index(g), starts, fam, units


def reads(repeat: int = 1, reverse: bool = False) -> list:
    """the fixture's reads: every unit alone, then COMBOS, each followed by its reverse complement; `repeat` times over, and `reverse`: in the opposite
    order -- the reads of a class then reach its kernel from the smallest need to the largest instead of the other way round"""
    _, _, _, _, units = genome()
    rows = []
    for fams in [[i] for i in range(len(FAMILIES))] + [list(c) for c in COMBOS]:
        x = units[fams[0]]
        for f in fams[1:]:
            x = np.concatenate([x, np.array([4], np.uint8), units[f]])
        rows += [x.copy(), synth.revcomp(x)]
    rows = rows * repeat
    return rows[::-1] if reverse else rows


def expected_need(max_occ: int = 500) -> np.ndarray:
    """sum(min(copies, max_occ)) over the units of every read of reads()"""
    per = [sum(min(FAMILIES[f], max_occ) for f in fams) for fams in [[i] for i in range(len(FAMILIES))] + [list(c) for c in COMBOS]]
    return np.repeat(np.array(per, np.int64), 2)


def contig_table(n: int) -> list:
    """the genome cut into n sequences [(name, length)]: the cuts alternate between the middle of a spacer and the middle of a unit copy (that occurrence then
    bridges two sequences and is dropped, src/bwamem.c:437), evenly spread over the copies"""
    g, _, starts, _, _ = genome()
    pick = np.linspace(0, len(starts) - 1, n + 1).astype(np.int64)[1:-1]
    cuts = [int(starts[j]) + UNIT // 2 if k & 1 else int(starts[j]) - 15 for k, j in enumerate(pick)]
    edges = [0] + cuts + [len(g)]
    assert all(b > a for a, b in zip(edges, edges[1:]))
    return [(f"c{k}", b - a) for k, (a, b) in enumerate(zip(edges, edges[1:]))]


def class_of(need: int) -> int:
    for c, cap in enumerate(CLASS_CAPS):
        if need <= cap:
            return c
    return N_CLASSES - 1


def classify(seeds: dict, lens, max_occ: int = 500, heavy: int = DEFAULT_HEAVY):
    """chain_classify_kernel on the host, from the seeds of seeds_to_host (score: the occurrence count of a group at the group's first seed).
    Returns (need [n_reads], where [n_reads], counts [16]): where = class c as c, lane bin b as -1 - b, a long read as N_CLASSES;
    counts = the 11 class counts, the 4 bin counts, the long reads."""
    n_ref, prefix, score = (np.asarray(seeds[k]).astype(np.int64) for k in ("n_ref_pos", "prefix", "score"))
    n_reads = len(lens)
    need = np.zeros(n_reads, np.int64); where = np.zeros(n_reads, np.int64); counts = np.zeros(16, np.uint32)
    for r in range(n_reads):
        n = int(n_ref[r]); nd = n
        if n > max_occ:                                 # only then can a group exceed max_occ
            nd, i = 0, 0
            while i < n:
                cnt = int(score[prefix[r] + i])
                if cnt == 0:
                    break
                nd += min(cnt, max_occ); i += cnt
        if int(lens[r]) > MAX_READ_LEN:
            nd = max(nd, heavy + 1); where[r] = N_CLASSES; counts[15] += 1
        elif nd > heavy:
            c = class_of(nd)
            if c < N_SUB and n > nd:                    # the four-per-wave classes stage the LOCATED seeds: such a read goes by that count
                c = min(class_of(n), N_SUB)
            where[r] = c; counts[c] += 1
        else:
            b = sum(nd > cap for cap in BIN_CAPS)
            where[r] = -1 - b; counts[N_CLASSES + b] += 1
        need[r] = nd
    return need, where, counts
