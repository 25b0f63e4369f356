"""The seeding kernels (csrc/seed_kernels.hip) on the case table of tests/seed_cases.py, in every form: bmh_seed_batch's output must equal
tests/golden/seed_cases.npz -- what the REFERENCE returned for the case, not the oracle beside the kernels -- under common.assert_seeds_equal, the
number of SMEMs must agree, and without the K-mer bitmap the number of candidates is the restated one.  Everything exact.

Forms: the index without the text, with it and the bitmap on or off, suffix-array samples of every 16th, 4th and 1st row; the backward search in one
launch, a phase per step and nine phases (the code keeps seven); the forward deal (knob SEED_FWD_SORT) by a previous call's counts; the fused form in a
child process; one workspace for the whole table, in order and back; the candidate list's capacity rule; the length limit; re-seeding."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import common
import seed_cases

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def bases():
    """the most bases a case of the table has"""
    return max(int(seed_cases.get(n).lens.sum()) for n in ("capacity_2000", "long_polyA", "pack_len_993_mixed"))


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()           # raises if the HIP extension is missing: no fallback
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


@pytest.fixture(scope="module")
def golden():
    return seed_cases.load_fixture()


class Indexes:
    """the device forms of the two genomes' indexes, made on demand, freed at the end of the module"""

    def __init__(self, B):
        self.B, self.made = B, {}

    def get(self, genome, text, kbits, intv):
        from test_seed_kmer_filter import _index
        key = (genome, text, kbits, intv)
        if key not in self.made:
            w = seed_cases.world(genome)
            d = _index(self.B, w.idx, w.g if text else None, kbits=kbits, whole_sa=False)
            if intv != 16:
                d.densify_sa(intv)
            assert (d.kbits_info()[0] > 0) == bool(text and kbits)
            self.made[key] = d
        return self.made[key]

    def free(self):
        for d in self.made.values():
            d.free()
        self.made = {}


@pytest.fixture(scope="module")
def indexes(hip):
    ix = Indexes(hip)
    yield ix
    ix.free()


def on_device(c):
    """the case's batch in HBM: the ASCII tensor is a view at byte offset c.shift of its allocation"""
    import torch
    buf = torch.full((c.shift + len(c.ascii) + 8,), ord("#"), dtype=torch.uint8, device="cuda")
    if len(c.ascii):
        buf[c.shift:c.shift + len(c.ascii)] = torch.from_numpy(c.ascii).cuda()
    r = buf[c.shift:]
    assert r.data_ptr() % 4 == c.shift % 4
    o = torch.from_numpy(c.offs.astype(np.int64)).to(torch.int32).cuda()
    l = torch.from_numpy(c.lens.astype(np.int64)).to(torch.int32).cuda()
    return r, o, l


def run_case(ws, dindex, c, reseed=None):
    from bwamem_hip.lib import seeds_to_host
    r, o, l = on_device(c)
    s = ws.seed_batch(dindex, r, o, l, c.msl, reseed=reseed)
    out = seeds_to_host(s, len(c.lens))
    out["n_smems"], out["n_cands"] = int(s.n_smems), int(s.n_cands)
    return out


def check(c, got, golden, bitmap, what=""):
    want = golden[c.name]
    common.assert_seeds_equal(got, want, f"{what}{c.name}: ")
    assert got["n_smems"] == want["n_smems"], (what, c.name)
    if not bitmap:
        assert got["n_cands"] == c.R.n_cands, (what, c.name, got["n_cands"], c.R.n_cands)


def run_table(hip, indexes, golden, text, kbits, intv, names=seed_cases.NAMES, what="", back=True):
    """one workspace for the whole table, in order (the packed buffers grow from 40-base to 65 535-base reads, the occurrence arrays from 64) and back"""
    ws = hip.SeedWorkspace(300, bases(), max_cands=bases(), max_occ=64)
    try:
        for name in tuple(names) + (tuple(names)[::-1] if back else ()):
            c = seed_cases.get(name)
            check(c, run_case(ws, indexes.get(c.genome, text, kbits, intv), c), golden, bool(text and kbits), what)
    finally:
        ws.free()


FORMS = {"notext_sa16": (False, False, 16), "text_bitmap_sa1": (True, True, 1), "text_nobitmap_sa4": (True, False, 4), "text_bitmap_sa16": (True, True, 16)}


@pytest.mark.parametrize("form", FORMS)
def test_table_in_every_index_form(hip, indexes, golden, form):
    run_table(hip, indexes, golden, *FORMS[form], what=form + ": ")


@pytest.mark.parametrize("phases", ["1", "1,2,3,4,5,6,7,8,9", "3,1000"])
def test_backward_phases(hip, indexes, golden, phases):
    """a phase per step; nine entries, two more than the code keeps; a phase long enough to end every walk of the table"""
    old = os.environ.get("BMH_SEED_BWD_PHASES")
    os.environ["BMH_SEED_BWD_PHASES"] = phases
    try:
        run_table(hip, indexes, golden, True, False, 1, what="phases " + phases + ": ", back=False)
    finally:
        if old is None:
            os.environ.pop("BMH_SEED_BWD_PHASES", None)
        else:
            os.environ["BMH_SEED_BWD_PHASES"] = old


def test_forward_deal_by_the_previous_calls_counts(hip, indexes, golden):
    """SEED_FWD_SORT: the second call of a batch deals its reads by the first call's iteration counts, a batch of another read count deals plainly"""
    L = hip.load_library()
    ws = hip.SeedWorkspace(300, bases(), max_cands=bases(), max_occ=64)
    L.bmh_tune_set(b"SEED_FWD_SORT", 1, 0)
    try:
        for name in ("pack_count_257", "pack_count_257", "stairs", "stairs", "filter_far", "pack_len_993_mixed", "pack_len_993_mixed", "long_polyA", "long_polyA",
                     "pack_count_65", "mixed_msl19", "mixed_msl19", "pack_count_257"):
            c = seed_cases.get(name)
            check(c, run_case(ws, indexes.get(c.genome, False, False, 16), c), golden, False, "dealt: ")
    finally:
        L.bmh_tune_set(b"SEED_FWD_SORT", 0, 1)
        ws.free()


def test_fused_form_in_a_child(hip):
    """BMH_SEED_FUSED is read once per process: the whole table once in a fresh child (long_polyA fills the scratch depth max_len - min_seed_len + 1 exactly)"""
    if os.environ.get("BMH_CHILD"):
        pytest.skip("already inside a child")
    env = dict(os.environ, BMH_SEED_FUSED="1", BMH_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__) + "::test_table_in_every_index_form[notext_sa16]"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def test_capacity_one_candidate_per_base_holds_every_legal_batch(hip, indexes, golden):
    """57 poly-A reads of 2 000 bases and 7 empty ones take 119 808 slots for 112 974 candidates: a workspace sized with one candidate per base holds them"""
    c = seed_cases.get("capacity_2000")
    bases = int(c.lens.sum())
    assert c.R.slots > bases + (64 // 64 + 1) * (seed_cases.CAND_CHUNK + 64)
    ws = hip.SeedWorkspace(64, bases, max_cands=bases, max_occ=64)
    try:
        check(c, run_case(ws, indexes.get("small", False, False, 16), c), golden, False)
    finally:
        ws.free()


def test_a_small_candidate_list_is_refused_and_the_workspace_lives_on(hip, indexes, golden):
    """BMH_ECAPACITY with its message (every write of the kernels is guarded by the capacity); the next call on a roomy workspace and the next small batch
    on the same one are right"""
    big, small = seed_cases.get("capacity_500"), seed_cases.get("text_edges")
    ws = hip.SeedWorkspace(64, bases(), max_cands=1000, max_occ=64)
    roomy = hip.SeedWorkspace(64, bases(), max_cands=bases(), max_occ=64)
    try:
        with pytest.raises(RuntimeError, match=r"rc=-3: .*candidate slots > capacity"):
            run_case(ws, indexes.get("small", False, False, 16), big)
        check(big, run_case(roomy, indexes.get("small", False, False, 16), big), golden, False)
        check(small, run_case(ws, indexes.get("main", False, False, 16), small), golden, False)
        with pytest.raises(RuntimeError, match=r"rc=-3: .*candidate slots > capacity"):
            run_case(ws, indexes.get("small", False, False, 16), big)
        check(small, run_case(ws, indexes.get("main", False, False, 16), small), golden, False)
    finally:
        ws.free(); roomy.free()


def test_a_read_of_65536_bases_is_refused(hip, indexes, golden):
    """BMH_EINVAL before any seeding kernel runs; the workspace takes the next batch"""
    import torch
    ws = hip.SeedWorkspace(64, bases(), max_cands=bases(), max_occ=64)
    d = indexes.get("main", False, False, 16)
    r = torch.full((65536 + 8,), ord("A"), dtype=torch.uint8, device="cuda")
    o = torch.zeros(2, dtype=torch.int32, device="cuda")
    l = torch.tensor([40, 65536], dtype=torch.int32, device="cuda")
    try:
        with pytest.raises(RuntimeError, match=r"rc=-2: .*longer than 65535"):
            ws.seed_batch(d, r, o, l, 19)
        c = seed_cases.get("text_edges")
        check(c, run_case(ws, d, c), golden, False)
    finally:
        ws.free()


def test_reseeding_on_the_table(hip, indexes):
    """rounds 2 and 3 (ReseedOpt.default(enable=1)) against the reference's bwt_smem1 / bwt_seed_strategy1 walk of tests/test_reseed.py, where the reference's
    library travelled with the tree.  Without long_polyA: the reference's own walk takes 43 s on the 65 535-base read (rounds 2 and 3 start a search at
    every base of the run)"""
    import oracle_py
    if not oracle_py.Ref.available():
        pytest.skip("oracle/_ref/libref.so not built")
    from bwamem_hip.lib import ReseedOpt
    from test_reseed import ref_seeds
    ref, bwts = oracle_py.Ref(), {}
    ws = hip.SeedWorkspace(300, bases(), max_cands=bases(), max_occ=64)
    try:
        for name in seed_cases.NAMES:
            if name == "long_polyA":
                continue
            c = seed_cases.get(name)
            if c.genome not in bwts:
                bwts[c.genome] = ref.bwt_from_index(seed_cases.world(c.genome).idx)
            want = ref_seeds(ref, bwts[c.genome], c.all_codes, c.offs, c.lens, k=c.msl, reseed={})
            got = run_case(ws, indexes.get(c.genome, True, True, 1), c, reseed=ReseedOpt.default(enable=1))
            common.assert_seeds_equal(got, want, f"re-seeding, {name}: ")
            assert got["n_smems"] == want["n_smems"], name
    finally:
        ws.free()
