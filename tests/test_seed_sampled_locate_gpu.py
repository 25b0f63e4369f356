"""Sampled locate (bmh_seed_ws_set_sample, csrc/seed_kernels.hip: expand_locate_kernel): a batch that holds, of every SMEM group, only the
occurrences chaining with the same max_occ reads must be the complete batch in those slots, in every count and in the regions that come out of
chaining; bmh_seeds_locate_all must make it the complete batch.  Everything exact, against the same library with the sample off.

The text is 50 000 random bases with planted exact repeats: every 40-base unit occurs a chosen number of times, each copy between flanks that keep
a read's neighbouring unit from matching on, so a read made of units has one SMEM per unit with exactly that many occurrences (the full run's group
heads are checked against the plan).  Shapes: with max_occ 5 groups of 4, 5 (no sampling), 6 (step 1, the tail dropped), 9 (step 1), 10 (step 2
exact), 11 (step 2, remainder) and 70 (the wave path beyond 64 lanes, step 14); with max_occ 2 groups of 3 and 4 (the lane path, groups of at most 4,
with sampling) and 70; a read with two groups of 70 and one of 3 between them; a poly-A unit, whose rows are the first a pattern can reach;
a batch without a group above max_occ.  (No group can begin at row 0 of the suffix array: that row is the sentinel's, an interval begins at
L2[c] + 1 or later; the kernel keeps locate_kernel's row-0 value all the same.)"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_seed_sample_rule import sampled_slots

pytestmark = pytest.mark.gpu

UNIT, TEXT, GAP = 40, 50_000, 130
# unit name -> copies in the text.  "l", "m", "r": the units of the three-group read (they occur nowhere next to each other)
COPIES = {"u4": 4, "u5": 5, "u6": 6, "u9": 9, "u10": 10, "u11": 11, "u70": 70, "l": 70, "m": 3, "r": 70, "polyA": 6}
READS = {"s4": ("u4",), "s5": ("u5",), "s6": ("u6",), "s9": ("u9",), "s10": ("u10",), "s11": ("u11",), "s70": ("u70",), "s3": ("m",),
         "three": ("l", "m", "r"), "polyA": ("polyA",)}
# case -> (reads of the batch, max_occ of the sample and of the chaining)
CASES = {
    "m5_every_shape": (("s4", "s5", "s6", "s9", "s10", "s11", "s70", "three", "polyA"), 5),
    "m5_three_groups_alone": (("three",), 5),
    "m2_lane_path": (("s3", "s4", "s70"), 2),
    "m5_nothing_above": (("s4", "s5", "s3"), 5),
    "m500_default": (("s70", "three", "s11"), 500),
    "m1_heads_only": (("s3", "s70", "three"), 1),
}


@functools.lru_cache(maxsize=1)
def planted():
    """(text, {unit: bases}): the units' copies dealt over slots GAP bases apart, in a random order"""
    rng = np.random.default_rng(20250)
    g = rng.integers(0, 4, TEXT).astype(np.uint8)
    units = {k: rng.integers(0, 4, UNIT).astype(np.uint8) for k in COPIES}
    units["polyA"] = np.zeros(UNIT, np.uint8)
    # the base a copy's flank must not be: what the read has there (its neighbouring unit), and for poly-A another A
    bad_left = {"m": units["l"][-1], "r": units["m"][-1], "polyA": 0}
    bad_right = {"l": units["m"][0], "m": units["r"][0], "polyA": 0}
    slots = [k for k, c in COPIES.items() for _ in range(c)]
    assert 100 + GAP * len(slots) + UNIT < TEXT
    for at, i in enumerate(rng.permutation(len(slots))):
        k, p = slots[i], 100 + GAP * at
        g[p:p + UNIT] = units[k]
        for q, bad in ((p - 1, bad_left.get(k)), (p + UNIT, bad_right.get(k))):
            if bad is not None:
                g[q] = (int(bad) + 1 + int(rng.integers(0, 3))) % 4
    return g, units


def batch_of(names):
    _, units = planted()
    return [np.concatenate([units[u] for u in READS[n]]) for n in names]


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()           # raises if the HIP extension is missing: no fallback
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.fixture(scope="module")
def world(hip):
    """the text's index on the device, with the whole suffix array and with every 16th row"""
    from bwamem_hip import fmindex
    from chain_case import _pack_pac
    g, _ = planted()
    idx = fmindex.build_fmd_index(g)
    dense = hip.Index.upload(idx, pac=_pack_pac(g), l_pac=len(g))
    dense.densify_sa(1)
    sparse = hip.Index.upload(idx, pac=_pack_pac(g), l_pac=len(g))
    yield {"dense": dense, "sparse": sparse}
    dense.free(); sparse.free()


def on_device(reads):
    import torch
    import common
    from bwamem_hip import synth
    flat, offs, lens = common.ragged_reads(reads)
    r = torch.from_numpy(synth.codes_to_ascii(flat)).cuda()
    o = torch.from_numpy(offs.astype(np.int64)).to(torch.int32).cuda()
    l = torch.from_numpy(lens.astype(np.int64)).to(torch.int32).cuda()
    return r, o, l, int(flat.size)


def workspace(hip, n, bases, sample):
    return hip.SeedWorkspace(n, bases, max_cands=max(bases, 64), max_occ=1 << 14, sample_max_occ=sample)


def state(hip, s):
    return int(hip.load_library().bmh_seeds_sample_state(C.byref(s)))


def raw(s, n_reads):
    """the arrays as they stand in HBM: no completion on the way (seeds_to_host completes)"""
    import torch
    from bwamem_hip.lib import _memcpy_d2d

    def rd(ptr, n, dt, tdt):
        if n == 0:
            return np.zeros(0, dt)
        buf = torch.empty(n, dtype=tdt, device="cuda")
        _memcpy_d2d(buf.data_ptr(), ptr, n * buf.element_size())
        return buf.cpu().numpy().view(dt)
    ns = int(s.n_seeds)
    return dict(rbeg=rd(s.d_rbeg, ns, np.uint64, torch.int64), qbeg=rd(s.d_qbeg, 2 * ns, np.int32, torch.int32).reshape(-1, 2),
                score=rd(s.d_score, ns, np.uint32, torch.int32), n_ref_pos=rd(s.d_n_ref_pos, n_reads, np.uint32, torch.int32),
                prefix=rd(s.d_prefix, n_reads, np.uint32, torch.int32))


FILL = 0xEE


def fill(s):
    """FILL into every byte of the three occurrence arrays"""
    import torch
    from bwamem_hip.lib import _memcpy_d2d
    ns = int(s.n_seeds)
    if ns:
        src = torch.full((8 * ns,), FILL, dtype=torch.uint8, device="cuda")
        _memcpy_d2d(s.d_rbeg, src.data_ptr(), 8 * ns); _memcpy_d2d(s.d_qbeg, src.data_ptr(), 8 * ns); _memcpy_d2d(s.d_score, src.data_ptr(), 4 * ns)
        torch.cuda.synchronize()


def groups(full):
    """[(first slot, occurrences)] of a complete batch, read by read"""
    out = []
    for p, n in zip(full["prefix"].tolist(), full["n_ref_pos"].tolist()):
        i = p
        while i < p + n:
            c = int(full["score"][i])
            assert c > 0
            out.append((i, c)); i += c
        assert i == p + n
    return out


def regions(hip, dindex, r, o, l, s, max_occ, one_call):
    """the regions of the batch from seeds s: bmh_chain_extend_merge, or bmh_chain_batch + bmh_chain_extend + bmh_chain_merge"""
    import torch
    from bwamem_hip.lib import ChainOpt, ChainWorkspace
    opt = ChainOpt(); hip.load_library().bmh_chain_opt_default(C.byref(opt))
    opt.max_occ = max_occ
    cw = ChainWorkspace(int(l.numel()), max(int(s.n_seeds), 1), opt=opt)
    cw.set_materialize(False)
    try:
        if one_call:
            regs = torch.full((4096, 8), -9, dtype=torch.int32, device="cuda")
            dj = cw.extend_merge(dindex, r, o, l, s, regs)
        else:
            dj = cw.chain_batch(dindex, r, o, l, s)
            out3 = torch.zeros(max(int(dj.n_jobs), 1), 3, dtype=torch.int32, device="cuda")
            regs = torch.full((max(int(dj.n_regs), 1), 8), -9, dtype=torch.int32, device="cuda")
            cw.extend(out3)
            cw.merge(out3, regs)
        torch.cuda.synchronize()
        return int(dj.n_jobs), regs.cpu().numpy()[: int(dj.n_regs)].copy()
    finally:
        cw.free()


def assert_same_regions(a, b, what):
    assert a[0] == b[0] and a[1].shape == b[1].shape and np.array_equal(a[1], b[1]), what
    assert len(a[1]) > 0, what


@pytest.mark.parametrize("case", list(CASES))
def test_sampled_batch_is_the_full_batch_where_chaining_reads(hip, world, case):
    from bwamem_hip.lib import seeds_to_host
    names, M = CASES[case]
    reads = batch_of(names)
    r, o, l, bases = on_device(reads)
    n, d = len(reads), world["dense"]
    ws_full, ws_smp = workspace(hip, n, bases, 0), workspace(hip, n, bases, M)
    try:
        sf = ws_full.seed_batch(d, r, o, l, 19)
        assert state(hip, sf) == 0
        full = raw(sf, n)
        # the text does what the plan says: one group per unit, with the unit's copies
        want_groups = [COPIES[u] for nm in names for u in READS[nm]]
        G = groups(full)
        assert [c for _, c in G] == want_groups and int(sf.n_smems) == len(G) and int(sf.n_seeds) == sum(want_groups)
        assert (case in ("m5_nothing_above", "m500_default")) == all(c <= M for _, c in G)
        assert ws_full.timing()["locate"] > 0

        # ---- the sampled batch, over arrays filled with a pattern: counts, heads, sampled slots; the other slots untouched
        ss = ws_smp.seed_batch(d, r, o, l, 19)
        fill(ss)
        ptrs = (ss.d_rbeg, ss.d_qbeg, ss.d_score)
        ss = ws_smp.seed_batch(d, r, o, l, 19)
        assert (ss.d_rbeg, ss.d_qbeg, ss.d_score) == ptrs
        assert state(hip, ss) == M
        tm = ws_smp.timing()
        # slot [5] spans no kernel in this form: what is left is the distance of two event records on one stream, microseconds (0.1 ms is room to spare)
        assert 0 < tm["locate"] < 0.1 and tm["expand"] > 0
        assert (int(ss.n_seeds), int(ss.n_smems), int(ss.n_cands)) == (int(sf.n_seeds), int(sf.n_smems), int(sf.n_cands))
        smp = raw(ss, n)
        assert np.array_equal(smp["n_ref_pos"], full["n_ref_pos"]) and np.array_equal(smp["prefix"], full["prefix"])
        written = np.zeros(int(sf.n_seeds), bool)
        for i, c in G:
            written[[i + u for u in sampled_slots(c, M)]] = True
            assert smp["score"][i] == c == full["score"][i]
        assert written.sum() == sum(min(c, M) if c > M else c for _, c in G)
        for k in ("rbeg", "qbeg", "score"):
            assert np.array_equal(smp[k][written], full[k][written]), (case, k)
        untouched = ~written
        assert (smp["rbeg"][untouched] == np.uint64(int.from_bytes(bytes([FILL]) * 8, "little"))).all()
        assert (smp["score"][untouched] == np.uint32(int.from_bytes(bytes([FILL]) * 4, "little"))).all()
        assert (smp["qbeg"][untouched].view(np.uint32) == np.uint32(int.from_bytes(bytes([FILL]) * 4, "little"))).all()

        # ---- regions from the sampled seeds, chained with max_occ = M: the full seeds' (both call forms); the seeds stay sampled
        for one_call in (True, False):
            assert_same_regions(regions(hip, d, r, o, l, ss, M, one_call), regions(hip, d, r, o, l, sf, M, one_call), (case, one_call))
            assert state(hip, ss) == M

        # ---- completion: every array is the full run's, the state 0, a second call a no-op
        L = hip.load_library()
        assert L.bmh_seeds_locate_all(C.byref(ss), None) == 0 and state(hip, ss) == 0
        done = raw(ss, n)
        for k in full:
            assert np.array_equal(done[k], full[k]), (case, k)
        assert L.bmh_seeds_locate_all(C.byref(ss), None) == 0
        assert all(np.array_equal(raw(ss, n)[k], full[k]) for k in full)

        # ---- seeds sampled with M, chained with another max_occ: completed by the chaining call itself, regions the full seeds'
        for one_call in (True, False):
            ss = ws_smp.seed_batch(d, r, o, l, 19)
            assert state(hip, ss) == M
            assert_same_regions(regions(hip, d, r, o, l, ss, 7, one_call), regions(hip, d, r, o, l, sf, 7, one_call), (case, "max_occ 7", one_call))
            assert state(hip, ss) == 0
            assert all(np.array_equal(raw(ss, n)[k], full[k]) for k in full)

        # ---- seeds_to_host completes
        ss = ws_smp.seed_batch(d, r, o, l, 19)
        host = seeds_to_host(ss, n)
        assert state(hip, ss) == 0 and all(np.array_equal(host[k], full[k]) for k in full)
    finally:
        ws_full.free(); ws_smp.free()


def test_forms_that_stay_complete(hip, world):
    """suffix-array samples of every 16th row, and the re-seeding entry: every slot filled, the state 0, whatever the workspace's sample"""
    from bwamem_hip.lib import ReseedOpt
    names, M = CASES["m5_every_shape"]
    reads = batch_of(names)
    r, o, l, bases = on_device(reads)
    n = len(reads)
    ws_full, ws_smp = workspace(hip, n, bases, 0), workspace(hip, n, bases, M)
    try:
        full = raw(ws_full.seed_batch(world["dense"], r, o, l, 19), n)
        s16 = ws_smp.seed_batch(world["sparse"], r, o, l, 19)
        fill(s16)
        s16 = ws_smp.seed_batch(world["sparse"], r, o, l, 19)
        assert state(hip, s16) == 0 and ws_smp.timing()["locate"] > 0
        got = raw(s16, n)
        assert all(np.array_equal(got[k], full[k]) for k in full)
        on = ReseedOpt.default(enable=1)
        want = raw(ws_full.seed_batch(world["dense"], r, o, l, 19, reseed=on), n)
        sr = ws_smp.seed_batch(world["dense"], r, o, l, 19, reseed=on)
        fill(sr)
        sr = ws_smp.seed_batch(world["dense"], r, o, l, 19, reseed=on)
        assert state(hip, sr) == 0
        got = raw(sr, n)
        assert all(np.array_equal(got[k], want[k]) for k in want) and len(want["rbeg"]) >= len(full["rbeg"])
        # and back: the next plain batch of the same workspace is sampled again
        assert state(hip, ws_smp.seed_batch(world["dense"], r, o, l, 19)) == M
    finally:
        ws_full.free(); ws_smp.free()


def test_records_of_no_workspace_are_left_alone(hip, world):
    """a hand-built bmh_seeds_t (its arrays belong to no workspace): the state 0, the completion a no-op; the same for a freed workspace's record"""
    import torch
    from bwamem_hip.lib import SeedsT
    L = hip.load_library()
    rb = torch.arange(6, dtype=torch.int64, device="cuda"); qb = torch.zeros(12, dtype=torch.int32, device="cuda")
    sc = torch.tensor([6, 0, 0, 0, 0, 0], dtype=torch.int32, device="cuda")
    nr = torch.tensor([6], dtype=torch.int32, device="cuda"); pf = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = SeedsT(6, 1, 1, rb.data_ptr(), qb.data_ptr(), sc.data_ptr(), nr.data_ptr(), pf.data_ptr())
    assert state(hip, s) == 0 and L.bmh_seeds_locate_all(C.byref(s), None) == 0
    torch.cuda.synchronize()
    assert rb.cpu().tolist() == list(range(6)) and sc.cpu().tolist() == [6, 0, 0, 0, 0, 0]
    reads = batch_of(("s70",))
    r, o, l, bases = on_device(reads)
    ws = workspace(hip, 1, bases, 5)
    ss = ws.seed_batch(world["dense"], r, o, l, 19)
    assert state(hip, ss) == 5
    ws.free()
    assert state(hip, ss) == 0 and L.bmh_seeds_locate_all(C.byref(ss), None) == 0
