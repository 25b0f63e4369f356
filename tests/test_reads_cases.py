"""The case table of tests/reads_cases.py on the CPU: the host walker (bmh_walk_record behind read_reads_files(host=True)) against what the reference's
kseq_read returned for every case (tests/golden/reads_input/cases_expected.npz), in every compressed form; the refusals with their messages; the plain
model of kseq_read against both archives, and the walker against the model on the seeded corpus.  The device parser has the same table in
test_reads_cases_gpu.py."""
import collections
import hashlib
import os

import numpy as np
import pytest

import reads_cases
from reads_cases import LONG, SHORT_PAIRS
from test_reads_input import FIX, FIXTURES, bgzf, check_expected, fixture_text, forms, same_read_sets

from bwamem_hip.aligner import read_reads_files

CASES, REFUSALS, PAIRS = reads_cases.cases(), reads_cases.refusals(), reads_cases.pairs()
BLOCK = 37                                                   # BGZF payload of the short texts: members cut lines, CR LF pairs and headers


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(FIX, "cases_expected.npz"))


def write(tmp_path, name: str, data: bytes) -> str:
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def case_forms(tmp_path, name: str, text: bytes) -> dict:
    """forms() of test_reads_input, the BGZF of a short text in 37-byte members"""
    ff = forms(tmp_path, name, text)
    if name not in LONG:
        write(tmp_path, name + ".bgzf", bgzf(text, BLOCK))
    return ff


def check_model(E, key: str, records):
    """the model's records against the archive's entry, field for field"""
    P = reads_cases.packed(records)
    for f in ("names", "comments", "seq", "qual"):
        assert P[f] == bytes(E[f"{key}__{f}"]), (key, f)
    assert P["lens"] == E[key + "__lens"].tolist(), key


def check_records(records, rs, what):
    """rs (comments=True) against the model's records"""
    P = reads_cases.packed(records)
    nb = len(P["seq"])
    assert rs.lens.tolist() == P["lens"], what
    assert bytes(rs.ascii[:nb]) == P["seq"] and bytes(rs.name_blob) == P["names"] and bytes(rs.comments[0]) == P["comments"], what
    assert (rs.qual is None and not P["qual"]) or bytes(rs.qual[:nb]) == P["qual"], what


# ---------------------------------------------------------------------------------------------------------------- the table itself

def test_the_table_and_the_archive_agree(expected):
    keys = {k.rsplit("__", 1)[0] for k in expected.files}
    assert keys == set(CASES) | set(PAIRS)
    for name, (text, kind, route) in CASES.items():
        assert hashlib.sha1(text).digest() == bytes(expected[name + "__sha1"]), name
        assert (len(expected[name + "__qual"]) > 0) == (kind == "fq"), name
        assert len(expected[name + "__lens"]) > 0, name
    for name, (t1, t2) in PAIRS.items():
        assert hashlib.sha1(t1 + b"\0" + t2).digest() == bytes(expected[name + "__sha1"]), name
    assert not set(CASES) & set(REFUSALS)
    assert reads_cases.cases() == CASES and reads_cases.random_texts() == reads_cases.random_texts()       # generated the same every time


def test_declared_routes_are_the_flag_rules():
    """every case's route is what the flag rules of the parser's header comment give it, and both sides of every rule are there"""
    for name, (text, kind, route) in CASES.items():
        assert reads_cases.device_route(text) == route, name
    n = collections.Counter(route for _, _, route in CASES.values())
    assert n["device"] >= 40 and n["host"] >= 15, n


# ---------------------------------------------------------------------------------------------------------------- the model

def test_model_equals_the_recorded_kseq_read(expected):
    for name, (text, kind, route) in CASES.items():
        check_model(expected, name, reads_cases.kseq_model(text))
    for name, (t1, t2) in PAIRS.items():
        recs, short = reads_cases.pair_model(t1, t2)
        check_model(expected, name, recs)
        assert (short, len(recs) // 2) == SHORT_PAIRS.get(name, (None, len(recs) // 2)), name


def test_model_equals_the_fixtures_archive():
    E = np.load(os.path.join(FIX, "expected.npz"))
    for name in FIXTURES:
        check_model(E, name, reads_cases.kseq_model(fixture_text(name)))
    check_model(E, "r1.fq+r2.fq", reads_cases.pair_model(fixture_text("r1.fq"), fixture_text("r2.fq"))[0])
    assert {k.rsplit("__", 1)[0] for k in E.files} == set(FIXTURES) | {"r1.fq+r2.fq"}              # no share left out


def test_model_refuses_the_refusals():
    for name, (text, piece) in REFUSALS.items():
        assert reads_cases.model_outcome(text) == ("refused", piece), name


# ---------------------------------------------------------------------------------------------------------------- the host walker

@pytest.mark.parametrize("name", sorted(CASES))
def test_host_walker_equals_the_reference_in_every_form(tmp_path, expected, name):
    text = CASES[name][0]
    for tag, p in case_forms(tmp_path, name, text).items():
        rs = read_reads_files(p, comments=True, host=True)
        check_expected(expected, name, rs)
    bare = read_reads_files(write(tmp_path, "bare", text), host=True)               # without comments: none kept, the same reads
    assert bare.comments is None
    for k in ("ascii", "codes", "offs", "lens", "name_blob", "name_off", "qual"):
        x, y = getattr(bare, k), getattr(rs, k)
        assert (x is None and y is None) or np.array_equal(x, y), (name, k)


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_host_walker_two_files(tmp_path, expected, name):
    t1, t2 = PAIRS[name]
    f1, f2 = case_forms(tmp_path, name + ".1", t1), case_forms(tmp_path, name + ".2", t2)
    for a, b in (("plain", "plain"), ("gz", "plain"), ("bgzf", "gz2"), ("bgzf", "bgzf")):
        if name in SHORT_PAIRS:
            short, n_pairs = SHORT_PAIRS[name]
            first, other = (f1[a], f2[b]) if short == 0 else (f2[b], f1[a])
            with pytest.raises(ValueError) as ei:
                read_reads_files(f1[a], f2[b], comments=True, host=True)
            assert f"{first} ends before {other} (after {n_pairs} pairs)" in str(ei.value), (name, a, b)
            rs = ei.value.partial
            assert len(rs) == 2 * n_pairs
        else:
            rs = read_reads_files(f1[a], f2[b], comments=True, host=True)
        check_expected(expected, name, rs)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_host_walker_refuses(tmp_path, name):
    text, piece = REFUSALS[name]
    for tag, p in case_forms(tmp_path, name, text).items():
        with pytest.raises(ValueError) as ei:
            read_reads_files(p, comments=True, host=True)
        assert piece in str(ei.value), (name, tag)


# ---------------------------------------------------------------------------------------------------------------- the corpus

def test_the_corpus_does_not_hide_in_refusals():
    """with the seed committed: two thirds of the texts parse, and each route occurs 20 times among them"""
    n = collections.Counter()
    for text in reads_cases.random_texts():
        status, got = reads_cases.model_outcome(text)
        n[reads_cases.device_route(text) if status == "ok" else "refused"] += 1
    assert sum(n.values()) == 300 and 3 * (n["device"] + n["host"]) >= 2 * 300 and n["device"] >= 20 and n["host"] >= 20, n


def test_host_walker_equals_the_model_on_the_corpus(tmp_path):
    for i, text in enumerate(reads_cases.random_texts()):
        status, want = reads_cases.model_outcome(text)
        p = write(tmp_path, "t", text)
        if status == "refused":
            with pytest.raises(ValueError) as ei:
                read_reads_files(p, comments=True, host=True)
            assert want in str(ei.value), (i, text)
        elif not want:                                       # (no header byte in the text: no reads)
            assert len(read_reads_files(p, comments=True, host=True)) == 0, (i, text)
        else:
            check_records(want, read_reads_files(p, comments=True, host=True), (i, text))
            if i % 10 == 0:
                check_records(want, read_reads_files(write(tmp_path, "t.bgzf", bgzf(text, BLOCK)), comments=True, host=True), (i, text, "bgzf"))
