"""The seeding case table of tests/seed_cases.py, without a GPU.  The chain of evidence, every link exact: the reference's compiled bwt_smem1 / bwt_sa
(oracle/ref_harness.c through oracle_py.Ref.seed_reads) -> tests/golden/seed_cases.npz, what it returned for every case (seed_cases.make_fixture) ->
the oracle beside the kernels (Oracle.seed_reads) and the restated split pipeline (seed_cases.restate), here -> the kernels of csrc/seed_kernels.hip in
every form, in tests/test_seed_cases_gpu.py.  Where the reference's library was built the fixture is compared with it live as well."""
import numpy as np
import pytest

import common
import seed_cases


@pytest.fixture(scope="module")
def golden():
    return seed_cases.load_fixture()


def test_the_table_covers_what_it_is_for():
    cases = seed_cases.all_cases()
    assert {c.family for c in cases.values()} == set(seed_cases.FAMILIES)
    w = seed_cases.world()
    assert len(w.g) <= 160_000 and seed_cases.longest_runs(w.g) == [(seed_cases.RUN_AT, 65535)]
    by = lambda fam: [c for c in cases.values() if c.family == fam]
    assert {len(c.lens) for c in by("packing")} >= set(seed_cases.PACK_COUNTS)
    assert all(len(c.lens) <= 300 for c in cases.values())
    assert {int(l) for c in by("packing") for l in c.lens} >= set(seed_cases.PACK_LENGTHS)
    assert {c.shift for c in by("packing")} == {0, 1, 2, 3}
    assert {c.msl for c in by("options")} == {1, 12, 19, 25}
    assert sum(int(c.lens.max(initial=0)) == seed_cases.MAX_READ for c in cases.values()) == 1          # the 65 535-base read once
    # the staging predicate is true for some blocks and false for others, for each of its three reasons alone
    stages = {b for c in cases.values() for b in c.stage}
    assert {(True, True, True), (False, False, True), (True, False, True), (True, True, False)} <= stages, stages
    # the chunked appends: a case whose slots exceed one per base plus the slack the workspace had for them
    c = cases["capacity_2000"]
    assert c.R.slots == 119_808 and int(c.lens.sum()) + 2 * 1088 == 116_176 and c.R.n_cands == 112_974


@pytest.mark.parametrize("name", seed_cases.NAMES)
def test_every_must_holds_and_the_oracle_equals_the_reference_fixture(golden, name):
    c = seed_cases.get(name)
    assert all(c.must.values()), (name, [k for k, v in c.must.items() if not v])
    w = seed_cases.world(c.genome)
    want = golden[name]
    got = w.orc.seed_reads(w.f, c.all_codes if len(c.all_codes) else np.zeros(1, np.uint8), c.offs.astype(np.uint64), c.lens, min_seed_len=c.msl)
    common.assert_seeds_equal(got, want, name + ": oracle vs fixture: ")
    assert len(got["smem_k"]) == want["n_smems"]
    # the restatement's SMEMs are the oracle's; its candidate count is what the device reports without the bitmap
    R = c.R
    assert sorted(R.smems) == sorted(zip(got["smem_read"].tolist(), got["smem_qb"].tolist(), got["smem_qe"].tolist(), got["smem_k"].tolist(), got["smem_s"].tolist()))
    assert R.n_smems == want["n_smems"] and R.n_seeds == len(want["rbeg"])
    print(f"{name}: {len(c.lens)} reads, {R.n_cands} candidates, {R.slots} slots, {R.n_smems} SMEMs, {R.n_seeds} occurrences, {R.steps} backward steps")


@pytest.mark.parametrize("name", seed_cases.NAMES)
def test_live_reference_equals_the_fixture(ref, golden, name, _bwts={}):
    """where oracle/_ref/libref.so was built"""
    got = seed_cases.reference_seeds(ref, _bwts, seed_cases.get(name))
    common.assert_seeds_equal(got, golden[name], name + ": live reference vs fixture: ")
    assert int(got["n_smems"]) == golden[name]["n_smems"]


def test_an_edited_table_is_refused(tmp_path):
    z = dict(np.load(seed_cases.FIXTURE))
    z["stairs.digest"] = np.array("0" * 40)
    np.savez_compressed(tmp_path / "stale.npz", **z)
    with pytest.raises(AssertionError, match="seed_cases.py changed"):
        seed_cases.load_fixture(tmp_path / "stale.npz")
