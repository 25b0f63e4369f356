"""The CIGAR stage on the hand-made regions of tests/cigar_cases.py, without a GPU.  The chain of evidence, every link exact: the reference's compiled
mem_reg2aln (oracle/ref_tail_harness.cpp: ref_tail_reg2aln) -> tests/golden/cigar_cases.npz, what it returned for every job
(tests/golden/make_cigar_golden.py) -> oracle_reg2aln (oracle/cigar_oracle.c) on the same jobs, here -> the kernels of csrc/cigar_kernels.hip, in
tests/test_cigar_cases_gpu.py.  The reference does not return the global score: that word comes from the oracle, which is pinned here on every other
word of every job.  Where the reference's library was built the fixture is compared with it live as well.  The table's routing (which kind a job takes,
which rounds the band retry runs, which wave-per-region form ends up with it) is restated in cigar_cases and checked here by name."""
import os
import re

import numpy as np
import pytest

import cigar_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "cigar_cases.npz")

_NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _NT4[ord(_c)] = _NT4[ord(_c.lower())] = _i


def codes(read):
    return _NT4[np.frombuffer(bytes(read), np.uint8)]


def ksw_params(scoring):
    import oracle_py
    return oracle_py.KswParams(*scoring, 0, 5, 1)


@pytest.fixture(scope="module")
def golden():
    """key_of(job) -> the reference's row (read-only).  A table edited without regenerating the fixture is refused here."""
    z = np.load(FIXTURE)
    assert str(z["digest"]) == cc.digest(), "tests/cigar_cases.py changed: run tests/golden/make_cigar_golden.py where the reference's library can be built"
    return cc.unpack_rows(z)


@pytest.fixture(scope="module")
def ref_tail():
    import oracle_py
    oracle_py.build(ref=True)
    if not oracle_py.RefTail.available():
        pytest.skip("oracle/_ref/libref_tail.so not built (needs the reference's sources)")
    rt = oracle_py.RefTail()
    if not hasattr(rt.lib, "ref_tail_reg2aln"):
        pytest.skip("oracle/_ref/libref_tail.so has no ref_tail_reg2aln")
    return rt


_oracle_rows = {}


def oracle_rows(oracle):
    """key_of(job) -> oracle_reg2aln's dict(pos, is_rev, cigar, NM, MD, score) for every job the reference accepts, computed once"""
    if not _oracle_rows:
        for j in cc.fixture_jobs():
            b = cc.batch_of(j)
            _oracle_rows[cc.key_of(j)] = oracle.reg2aln(cc.PAC, cc.L_PAC, codes(j.read), j.qb, j.qe, j.rb, j.re, j.truesc, reg_w=j.reg_w, opt_w=b.opt_w,
                                                        params=ksw_params(b.scoring), cap=4096)
    return _oracle_rows


def expected_rows(oracle, golden):
    """what the device must give: the reference's row, and the score word from the oracle"""
    orc = oracle_rows(oracle)
    return {k: dict(r, score=orc[k]["score"]) for k, r in golden.items()}


def dp_seqs(j):
    """query and target as ksw_global2 gets them"""
    s = cc.TEXT[j.rb:j.re]
    q = codes(j.read)[j.qb:j.qe]
    return (np.ascontiguousarray(q[::-1]), np.ascontiguousarray(s[::-1])) if j.flip else (np.ascontiguousarray(q), np.ascontiguousarray(s))


_traces = {}


def traces(oracle):
    """key_of(job) -> (rounds [(w2, score)], exit, demoted, the wave-per-region form that ends up with the job or None): the restated loop of mem_reg2aln over
    the oracle's ksw_global2"""
    if not _traces:
        for j in cc.fixture_jobs():
            b = cc.batch_of(j)
            q, t = dp_seqs(j)
            p = ksw_params(b.scoring)
            a, bb = b.scoring[0], b.scoring[1]

            def score_of(w2, q=q, t=t, b=b, p=p, a=a, bb=bb):
                band = cc.band_of(b.scoring, len(q), len(t), w2)
                if band is None:
                    return int(np.where((q > 3) | (t > 3), -1, np.where(q == t, a, -bb)).sum())
                return oracle.global2(q, t, band[0], params=p, cap=4096)[0]

            rounds, how = cc.retry_trace(b.scoring, b.opt_w, len(q), len(t), j.truesc, j.reg_w, score_of)
            kind = j.route[3]
            demoted = kind.startswith("F") and rounds[0][1] < j.truesc - a and rounds[0][0] != b.opt_w << 2
            form = cc.slow_form(len(q), len(t)) if kind == "slow" or demoted else None
            _traces[cc.key_of(j)] = (rounds, how, demoted, form)
    return _traces


def test_the_digest_guards_the_fixture(golden):
    assert len(golden) == len(cc.fixture_jobs()) == len(cc.all_jobs()) - sum(1 for j in cc.all_jobs() if j.route[3] == "reject")
    assert len({cc.key_of(j) for j in cc.all_jobs()}) == len(cc.all_jobs())
    assert cc.L_PAC % 4 != 0 and len(cc.PAC) == (cc.L_PAC + 3) // 4 + 8
    f = np.arange(cc.L_PAC)
    assert np.array_equal((cc.PAC[f >> 2] >> ((~f & 3) << 1)) & 3, cc.GENOME)
    n = len(cc.all_jobs())
    assert 200 <= n <= 500, n
    long_ = [j for j in cc.all_jobs() if len(j.read) > 320]
    assert max(len(j.read) for j in long_) <= 1500
    # only the families that need more go beyond 320 bases: the splits of the slow forms, the sides of CG_LDS_MAX, the long form
    assert all(any(l.startswith(("demoted_qlen", "narrow_side", "wide_", "long_", "md_digits_4", "bridging")) for l in j.limits) for j in long_)
    assert os.path.getsize(FIXTURE) < 1 << 20


BOTH_STRANDS = ([f"{g}_ncol{n}" for g in ("gap", "del", "ins") for n in (31, 33, 47, 49, 79, 81, 159, 161, 255, 257)]
                + [f"qlen_ncol{q}" for q in (32, 33, 48, 49, 80, 81, 160, 161, 256, 257)]
                + [f"demoted_qlen{q}" for q in (64, 65, 128, 129, 192, 193, 320, 321, 512, 513, 704, 705)]
                + ["gate_below", "gate_at", "one_run_low", "score_at", "score_below", "exit_repeat", "exit_rounds", "exit_cap", "first_w2_cap", "reg_w_above_opt_w",
                   "window_sweep", "corner", "rows_left", "lead_del", "trail_del", "cols_left", "trail_ins", "equal_cost", "clip5", "clip3", "clip_both", "n_bases",
                   "md_digits_123", "md_digits_4", "mm_first_last", "mm_chunk_edges", "narrow_side704", "narrow_side705", "wide_qlen704", "wide_qlen705", "wide_rlen704",
                   "wide_rlen705", "long_form", "long_fast", "long_beyond_4w", "ops_fit", "ops_over", "md_fit", "md_over"])
ONE_STRAND = ("rb_0", "re_l_pac", "rb_l_pac", "re_2l_pac", "bridging", "empty", "inverted")


def test_every_limit_is_in_the_table_from_both_sides():
    have = {}
    for j in cc.all_jobs():
        for l in j.limits:
            have.setdefault(l, set()).add(j.flip)
    for l in BOTH_STRANDS:
        assert have.get(l) == {False, True}, (l, have.get(l))
    for l in ONE_STRAND:
        assert l in have, l
    by = {cc.key_of(j): j for j in cc.all_jobs()}
    kind = lambda key: by[key].route[3]
    ncol = lambda key: by[key].route[2]
    for s in "fr":
        # the kinds, each limit from both sides: through a gap's length ...
        for d, n, k in ((12, 31, "F2"), (13, 33, "F3"), (20, 47, "F3"), (21, 49, "F5"), (36, 79, "F5"), (37, 81, "F10"), (76, 159, "F10"), (77, 161, "F16"), (124, 255, "F16"),
                        (125, 257, "slow")):
            for g in ("del", "ins"):
                assert (ncol(f"kinds:{g}{d}/{s}"), kind(f"kinds:{g}{d}/{s}")) == (n, k)
        # ... and through n_col = qlen under a wider band
        for q, k in ((32, "F2"), (33, "F3"), (48, "F3"), (49, "F5"), (80, "F5"), (81, "F10"), (160, "F10"), (161, "F16"), (256, "F16"), (257, "slow")):
            j = by[f"kinds:qlen{q}/{s}"]
            assert j.qe - j.qb == q == j.route[2] and 2 * j.route[1] + 1 > q and j.route[3] == k
        # the gate of the one-run jobs, 2 (o + e - a), under the default scoring and where only one of the two gates opens
        assert kind(f"kinds:gate11/{s}") == "trivial" and kind(f"kinds:gate12/{s}") == "F2"
        for sname, open_, shut in (("ins_dear", (6, 1), (9, 3)), ("del_dear", (6, 1), (9, 3))):
            lo, hi = by[f"sc_{sname}:gate_below/{s}"], by[f"sc_{sname}:gate_at/{s}"]
            assert lo.route[3] == "trivial" and hi.route[3] == "F2" and hi.truesc == lo.truesc - 1
            assert cc.infer_bw(100, 100, hi.truesc, 1, *open_) > 0 and cc.infer_bw(100, 100, hi.truesc, 1, *shut) == 0
        # the retry limit is one score point wide
        lo, hi = by[f"retry:at_truesc_minus_a/{s}"], by[f"retry:below_truesc_minus_a/{s}"]
        assert hi.truesc == lo.truesc + 1 and len(lo.read) == len(hi.read)
    # the four ends of the text
    g = {j.name: j for j in cc.batches()["geometry"].jobs}
    assert g["rb_0/f"].rb == 0 and g["re_l_pac/f"].re == cc.L_PAC and g["rb_l_pac/r"].rb == cc.L_PAC and g["re_2l_pac/r"].re == 2 * cc.L_PAC
    assert {j.name for j in cc.all_jobs() if j.route[3] == "reject"} == {"bridging", "bridging_by_one", "empty_region", "inverted_region", "empty_query", "inverted_query",
                                                                          "bridging_long"}
    # the sides of CG_LDS_MAX
    for q in (704, 705):
        for s in "fr":
            assert g[f"narrow_qlen{q}/{s}"].qe == q and g[f"narrow_rlen{q}/{s}"].re - g[f"narrow_rlen{q}/{s}"].rb == q
            assert g[f"wide_qlen{q}/{s}"].qe == q and g[f"wide_rlen{q}/{s}"].re - g[f"wide_rlen{q}/{s}"].rb == q
    assert {cc.batches()[n].family for n in cc.batch_names()} == set(cc.FAMILIES)
    assert {b.scoring for b in cc.batches().values() if b.family == "scorings"} == set(cc.SCORINGS.values())
    assert {b.stride for b in cc.batches().values()} == {8, 16} and {b.opt_w for b in cc.batches().values()} == {4, 20, 100}


def test_every_kind_form_and_retry_exit_is_reached(oracle, golden):
    tr = traces(oracle)
    orc = oracle_rows(oracle)
    jobs = cc.fixture_jobs()
    kinds, forms, exits = {}, {}, {}
    for j in cc.all_jobs():
        kinds[j.route[3]] = kinds.get(j.route[3], 0) + 1
    for j in jobs:
        rounds, how, demoted, form = tr[cc.key_of(j)]
        assert rounds[-1][1] == orc[cc.key_of(j)]["score"], (cc.key_of(j), rounds)       # the restated loop ends where oracle_reg2aln ends
        if form:
            forms.setdefault(form, {"demoted": 0, "classified": 0})["demoted" if demoted else "classified"] += 1
        exits[(how, len(rounds))] = exits.get((how, len(rounds)), 0) + 1
        # what the table says a job is there for
        if "exit" in j.extra:
            assert (how, len(rounds)) == (j.extra["exit"], j.extra["rounds"]), (cc.key_of(j), rounds, how)
        if "form" in j.extra:
            assert form == j.extra["form"], (cc.key_of(j), form)
        for l in j.limits:
            if l.startswith("demoted_qlen"):
                assert demoted and form == cc.slow_form(int(l[12:]), int(l[12:])), (cc.key_of(j), demoted, form)
            if l == "score_at":
                assert rounds[0][1] == j.truesc - cc.batch_of(j).scoring[0] and not demoted and len(rounds) == 1, (cc.key_of(j), rounds)
            if l == "score_below" and j.route[3] != "trivial":
                assert rounds[0][1] == j.truesc - cc.batch_of(j).scoring[0] - 1 and demoted, (cc.key_of(j), rounds)
            if l == "first_w2_cap":
                assert rounds[0][0] == 4 * cc.batch_of(j).opt_w and rounds[0][1] < j.truesc - 1 and not demoted and len(rounds) == 1
            if l == "one_run_low":
                assert [r[0] for r in rounds] == [0, 0] and how == "repeat" and rounds[0][1] < j.truesc - 20
    print("kinds: " + ", ".join(f"{k} {kinds.get(k, 0)}" for k in cc.KINDS))
    print("wave-per-region forms: " + ", ".join(f"<{f}> {v['classified']} classified + {v['demoted']} demoted" for f, v in sorted(forms.items())))
    print("retry exits (how, rounds): " + ", ".join(f"{h} after {n}: {c}" for (h, n), c in sorted(exits.items())))
    assert set(kinds) == set(cc.KINDS)
    assert set(forms) == {name for _, name in cc.SLOW_FORMS} | {"long"}
    assert all(v["demoted"] >= 2 for v in forms.values())                         # each instantiation is reached by a demoted job on either strand
    assert {"5,3", "11,8", "long"} <= {f for f, v in forms.items() if v["classified"]}
    assert {("reached", 1), ("repeat", 2), ("rounds", 3), ("cap", 1), ("cap", 2), ("cap", 3)} <= set(exits)
    # demoted jobs on both sides of every split of the wave-per-region forms
    by = {cc.key_of(j): j for j in jobs}
    for lo, hi in ((64, 65), (128, 129), (192, 193), (320, 321), (512, 513), (704, 705)):
        for s in "fr":
            assert tr[f"retry:demoted{lo}/{s}"][3] != tr[f"retry:demoted{hi}/{s}"][3] and by[f"retry:demoted{lo}/{s}"].qe == lo


def test_oracle_equals_the_reference_fixture(oracle, golden):
    orc = oracle_rows(oracle)
    bad = [k for k in golden if not cc.same_row(orc[k], golden[k])]
    assert not bad, (len(bad), bad[:5], orc[bad[0]], golden[bad[0]])


def test_the_fixture_equals_the_live_reference(ref_tail, golden):
    """where oracle/_ref/libref_tail.so was built: mem_reg2aln itself on every job"""
    bad = [cc.key_of(j) for j in cc.fixture_jobs() if not cc.same_row(cc.reference_row(ref_tail, j), golden[cc.key_of(j)])]
    assert not bad, (len(bad), bad[:5])


def _cg(row):
    return "".join(f"{int(c) >> 4}{'MIDS'[int(c) & 0xf]}" for c in row["cigar"])


def test_the_traceback_cases_are_what_they_are_for(golden):
    trace = cc.batches()["trace"]
    for flip in (False, True):
        ev = set()
        for j in trace.jobs:
            if j.flip == flip:
                ev |= cc.finish_windows(cc.dp_ops(j, golden[cc.key_of(j)]), j.qe - j.qb, j.re - j.rb, j.route[1])
        print(("reverse" if flip else "forward") + " strand, window events: " + ", ".join(f"{s}:{e}" for s, e in sorted(ev)))
        assert ev >= {(s, e) for s in "EF" for e in ("enter_first", "enter_last", "leave_last", "inside", "corner")}, sorted(ev)
    row = lambda name: golden["trace:" + name]
    runs = lambda md: re.findall(r"\d+", md)
    job = {j.name: j for j in trace.jobs}
    for s in "fr":
        # a leading deletion moves POS, NM does not count it, MD drops it; a trailing one only goes
        fwd_pos = lambda j: 2 * cc.L_PAC - j.re if j.flip else j.rb
        assert _cg(row(f"lead_del6/{s}")) == "80M" and row(f"lead_del6/{s}")["pos"] == fwd_pos(job[f"lead_del6/{s}"]) + 6
        assert (row(f"lead_del6/{s}")["NM"], row(f"lead_del6/{s}")["MD"]) == (0, "80")
        assert _cg(row(f"trail_del6/{s}")) == "80M" and row(f"trail_del6/{s}")["pos"] == fwd_pos(job[f"trail_del6/{s}"]) and row(f"trail_del6/{s}")["MD"] == "80"
        assert _cg(row(f"lead_ins4/{s}")) == "4I80M" and _cg(row(f"trail_ins4/{s}")) == "80M4I"
        # equal cost: the left-most placement in DP coordinates, which for a region on the reverse half is the left-most on the forward genome too
        assert _cg(row(f"homo_del2/{s}")) == "40M2D48M" and _cg(row(f"dinuc_del2/{s}")) == "40M2D48M"
        # (the clips change sides with the strand)
        def clipped(c5, mid, c3):
            left, right = (c5, c3) if s == "f" else (c3, c5)
            return (f"{left}S" if left else "") + mid + (f"{right}S" if right else "")
        assert _cg(row(f"clip5_del4/{s}")) == clipped(7, "50M4D50M", 0) and _cg(row(f"clip3_del4/{s}")) == clipped(0, "50M4D50M", 9)
        assert _cg(row(f"clip_both_del4/{s}")) == clipped(11, "50M4D50M", 5) and _cg(row(f"clip_both_one_run/{s}")) == clipped(11, "100M", 5)
        assert row(f"n_del4/{s}")["NM"] == 8 and row(f"n_one_run/{s}")["NM"] == 3
        assert sorted(len(x) for x in re.findall(r"\d+", row(f"md_digits/{s}")["MD"])) == [1, 2, 3, 3] and runs(row(f"md_digits_one_run/{s}")["MD"]) == runs(row(f"md_digits/{s}")["MD"]) == ["5", "47", "130", "115"]
        md = row(f"mm_first_last/{s}")["MD"]
        assert re.fullmatch(r"0[ACGT]98[ACGT]0", md) and runs(row(f"mm_first_last_one_run/{s}")["MD"]) == runs(md)
        assert re.fullmatch(r"15[ACGT]0[ACGT]46[ACGT]0[ACGT]62[ACGT]0[ACGT]71", row(f"mm_chunk_edges/{s}")["MD"])
        assert runs(row(f"mm_chunk_edges_one_run/{s}")["MD"]) == runs(row(f"mm_chunk_edges/{s}")["MD"])
        assert 4 in {len(x) for x in re.findall(r"\d+", golden[f"long:del130_md4/{s}"]["MD"])} and golden[f"long:one_run_md4/{s}"]["MD"].startswith("1150")
    # the clips change sides with the strand
    assert _cg(golden["trace:clip5_one_run/f"]) == "7S100M" and _cg(golden["trace:clip5_one_run/r"]) == "100M7S"


def small_flags(b, j, row):
    """the flag word a job gets under the small slots of its batch: 1 where the walk meets more than max_cigar - 2 operations, 8 where the MD string and its NUL
    do not fit md_cap"""
    n_ops = len(cc.dp_ops(j, row))
    return (1 if n_ops > b.max_cigar - 2 else 0) | (8 if len(row["MD"]) + 1 > b.md_cap else 0)


def test_the_slot_cases_sit_on_their_limits(golden):
    b = cc.batches()["slots"]
    assert (b.max_cigar, b.md_cap) == (16, 24)
    seen = set()
    for j in b.jobs:
        row = golden[cc.key_of(j)]
        n_ops = len(cc.dp_ops(j, row))
        assert small_flags(b, j, row) == j.extra["small"], (j.name, _cg(row), row["MD"])
        if "ops" in j.extra:
            assert n_ops == j.extra["ops"] and len(row["MD"]) + 1 < b.md_cap, (j.name, _cg(row), row["MD"])
            seen.add(("ops", n_ops, len(row["cigar"]) - n_ops))
        if "md_len" in j.extra:
            assert len(row["MD"]) == j.extra["md_len"] and n_ops == 1
            seen.add(("md", len(row["MD"]), j.route[3] == "trivial"))
    # 14 operations and two clips fill the 16 slots, 15 do not fit; 23 characters and the NUL fill the 24 bytes, 24 do not fit -- with and without DP
    assert {("ops", 14, 2), ("ops", 14, 1), ("ops", 15, 0), ("ops", 16, 2), ("md", 23, False), ("md", 23, True), ("md", 24, False), ("md", 24, True)} <= seen
    # every wave of four regions in cigar_finish_kernel holds a flagged job beside one that fits
    flags = [j.extra["small"] for j in b.jobs]
    assert all(0 in flags[k:k + 4] for k in range(0, len(flags), 4)) and sum(1 for k in range(0, len(flags), 4) if any(flags[k:k + 4])) >= 4
