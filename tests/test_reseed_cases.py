"""The re-seeding case table of tests/reseed_cases.py, without a GPU.  The chain of evidence, every link exact: the reference's compiled bwt_smem1,
bwt_seed_strategy1 and bwt_sa under a restated mem_collect_intv (test_reseed.ref_seeds) -> tests/golden/reseed_cases.npz, what they returned for every case
(reseed_cases.make_fixture) -> the restatement of rounds 2 and 3 over the oracle's rank function (reseed_cases.restate), here -> the kernels of
csrc/reseed_kernels.hip, their counters and both launches of round 2, in tests/test_reseed_cases_gpu.py.  Where the reference's library was built the
fixture is compared with it live as well: the only test here that may skip."""
import numpy as np
import pytest

import common
import reseed_cases as rc


@pytest.fixture(scope="module")
def golden():
    return rc.load_fixture()


@pytest.mark.parametrize("name", rc.NAMES)
def test_every_must_holds_and_the_restatement_equals_the_reference_fixture(golden, name):
    c = rc.get(name)
    assert all(c.must.values()), (name, [k for k, v in c.must.items() if not v])
    S, want = c.S, golden[name]
    common.assert_seeds_equal(S.cols, want, name + ": restatement vs fixture: ")
    assert S.cols["n_smems"] == want["n_smems"] and list(S.rounds) == want["rounds"].tolist()
    # its first round alone (what a call with re-seeding off returns) is the project's oracle
    w = rc.world(c.genome)
    got = w.orc.seed_reads(w.f, c.all_codes if len(c.all_codes) else np.zeros(1, np.uint8), c.offs.astype(np.uint64), c.lens, min_seed_len=c.msl)
    common.assert_seeds_equal(S.cols1, got, name + ": first round vs oracle: ")
    assert S.cols1["n_smems"] == len(got["smem_k"]) == S.rounds[0]
    print(f"{name}: {len(c.lens)} reads, k {c.msl} split_len {c.split_len} split_width {c.sw} max_mem_intv {c.mi}: {S.n_tasks} tasks, {S.n_over} overflow, longest list "
          f"{int(S.lists.max(initial=0))}, groups per round {S.rounds}, round-3 seeds per read up to {int(S.r3_per_read.max(initial=0))}, {S.steps} rank steps, "
          f"{int(S.task_steps.max(initial=0))} in one task")


def test_live_reference_equals_the_fixture(ref, golden):
    """where oracle/_ref/libref.so was built"""
    bwts = {}
    for name in rc.NAMES:
        got = rc.reference_seeds(ref, bwts, rc.get(name))
        common.assert_seeds_equal(got, golden[name], name + ": live reference vs fixture: ")
        assert int(got["n_smems"]) == golden[name]["n_smems"] and got["rounds"].tolist() == golden[name]["rounds"].tolist(), name


def test_an_edited_table_is_refused(tmp_path):
    z = dict(np.load(rc.FIXTURE))
    z["list_32_33.digest"] = np.array("0" * 40)
    np.savez_compressed(tmp_path / "stale.npz", **z)
    with pytest.raises(AssertionError, match="reseed_cases.py changed"):
        rc.load_fixture(tmp_path / "stale.npz")
    # the options are part of a case: the same reads under another split_width are another case
    c = rc.get("list_32_33")
    other = rc.make_case(c.name, c.family, c.ascii, c.offs, c.lens, c.msl, c.genome, (c.sf, c.sw + 1, c.mi), {"the same reads": lambda c, S: True})
    assert other.digest != c.digest


def test_the_fixture_holds_data_only_and_stays_small():
    import os
    z = np.load(rc.FIXTURE, allow_pickle=False)
    assert all(z[f].dtype.kind in "iuU" for f in z.files)
    assert os.path.getsize(rc.FIXTURE) < 256 << 10


def test_the_table_covers_what_it_is_for():
    """every limit named here is read off the restatement's details, not off the builders' arguments"""
    cases = rc.all_cases()
    assert {c.family for c in cases.values()} == set(rc.FAMILIES)
    assert all(len(c.lens) <= 300 for c in cases.values())
    assert all(len(rc.world(g).g) <= 200_000 for g in {c.genome for c in cases.values()})
    by = lambda fam: [c for c in cases.values() if c.family == fam]
    tasks = [t for c in cases.values() for t in c.S.tasks]
    # select
    assert {c.S.n_tasks for c in by("select")} >= set(rc.TASK_COUNTS)
    for k in (15, 19, 23):
        lo, hi = cases["select_len_k%d_below" % k], cases["select_len_k%d_above" % k]
        assert hi.split_len == lo.split_len + 1 and np.nextafter(np.float32(lo.sf), np.float32(9)) == np.float32(hi.sf)
        for c in (lo, hi):
            assert {t.src[1] - t.src[0] for t in c.S.tasks} >= {c.split_len, c.split_len + 1}
            assert c.split_len - 1 in {g[1] - g[0] for d in c.S.reads for g in d.groups if g[4] == 1} - {t.src[1] - t.src[0] for t in c.S.tasks}
    assert {(t.src[0] + t.src[1]) & 1 for t in tasks} == {0, 1}
    mer_tasks = lambda c: {t.src[2] for t in c.S.tasks if t.src[1] - t.src[0] == 40} & set(rc.MER_COUNTS)
    for sw in (4, 64):                 # occurrences split_width (a task) and split_width + 1 (none), and the row in which split_width + 1 is one
        assert any(c.sw == sw and sw in mer_tasks(c) and sw + 1 not in mer_tasks(c) for c in by("options"))
        assert any(c.sw == sw + 1 and sw + 1 in mer_tasks(c) for c in by("options"))
    assert {2, 3, 5, 6, 64, 65, 66} <= {t.m for t in tasks} and max(t.m for c in by("options") for t in c.S.tasks) == 130
    # round 2, forward: the 32 | 33 pair, the overflow counts, the three endings
    assert {32, 33} <= set(cases["list_32_33"].S.lists.tolist()) and cases["list_32_33"].S.n_over == int((cases["list_32_33"].S.lists > 32).sum()) == 2
    assert {1, 64, 65} <= {c.S.n_over for c in by("forward")}
    assert any(c.S.n_over == c.S.n_tasks > 1 for c in by("forward")) and any(0 < c.S.n_over < c.S.n_tasks <= 64 for c in by("forward"))
    assert {t.fwd_end for t in tasks} == {"end", "N", "small"}
    assert {t.fwd_end for t in tasks if t.n_list > rc.CAP} == {"end", "N", "small"}
    assert max(t.n_list for t in tasks) > 256
    # round 2, backward: the three endings, the three ways an entry or a hit is dropped
    assert {t.bwd_end for t in tasks} == {"start", "N", "empty"}
    assert {t.bwd_end for t in tasks if t.n_list > rc.CAP} == {"start", "N", "empty"}
    for what in ("equal", "contained", "short"):
        assert sum(getattr(t, what) for t in tasks) > 0, what
    assert sum(t.behind for t in tasks) == 0           # (a shorter match occurs at least as often as a longer one: it never fails behind one that survives)
    assert any(rc.twice(c, c.S) for c in cases.values())
    # round 3
    assert {c.mi for c in by("round3")} >= {0, 1, 20}
    r3 = [d.r3 for c in cases.values() for d in c.S.reads if d.r3]
    assert any(d.carry for d in r3) and any(d.end_unpushed for d in r3) and any(d.n_mid for d in r3) and any(d.empty_returned for d in r3)
    pushed = {(c.mi, s) for c in by("options") for d in c.S.reads for b, e, _, s in d.r3.seeds if e - b == c.msl + 1}
    passed = {(c.mi, s) for c in by("options") for d in c.S.reads for s in d.r3.at_min} - pushed
    assert {(5, 4), (64, 63), (65, 64), (130, 129)} <= pushed                # max_mem_intv - 1 occurrences at min_seed_len + 1 bases: a seed
    assert {(4, 4), (5, 5), (63, 63), (64, 64), (65, 65), (129, 129)} <= passed      # max_mem_intv occurrences: extended further
    assert len(cases["r3_tiled_k19"].S.reads[0].r3.seeds) == 10 == 200 // 20
    # merge
    assert {len(c.lens) for c in by("merge")} >= {1, 2, 63, 64, 65, 257}
    assert any(sum(c.S.rounds) == 0 and len(c.lens) > 64 for c in by("merge"))
    assert any(g[0] > 32767 for d in cases["long_40000"].S.reads for g in d.groups)
    assert any(((c.S.groups_per_read[1:-1] == 0) & (c.S.groups_per_read[:-2] > 0) & (c.S.groups_per_read[2:] > 0)).any() for c in by("merge"))
    # options: every k with every row
    assert {(c.msl, c.sw, c.mi) for c in by("options")} == {(k, sw, mi) for k in (15, 19, 23) for _, sw, mi in rc.ROWS.values()}
    # cost
    assert all(int(c.S.task_steps.max(initial=0)) <= rc.MAX_TASK_STEPS and c.S.steps <= rc.MAX_CASE_STEPS for c in cases.values())
    assert max(int(c.S.task_steps.max(initial=0)) for c in cases.values()) > 50_000          # (the A-run read: the cap is approached, on purpose)
