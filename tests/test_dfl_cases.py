"""The one-wave DEFLATE compressor (csrc/deflate_core.h) on the case table of tests/dfl_cases.py, on the CPU: the library's host entry point and the same source
under AddressSanitizer and UBSan (tests/deflate_core_host.cpp, which also writes a trace: the form chosen, the bits estimated, the three length arrays and
their counts).  Every member inflates to its piece with zlib and with the repository's own inflater, holds the tokens the Python model of the tokenizer gives,
and meets the musts of its case; the three codes are complete; their cost is the Huffman optimum (heapq) where that fits the length limit and no less where it
does not; the estimate the form is decided from is the bits written.  The same table runs through the kernel in test_dfl_cases_gpu.py.

Cost / optimum of the codes the Kraft repair limited, as measured (no bound is asserted above 1; test_case prints them, see pytest -s):
  lit15: a literal ladder of depth 16                    literal / length   114896 / 114895
  lit15: a literal ladder of depth 18                    literal / length   394932 / 394924
  dist15: 18 distance symbols in a ladder of depth 16    distance            24590 /  24589      code length   664 / 647
  cl7: code lengths in a ladder of depth 8               code length           477 /    476
  spill 694 / 693, tok48 958 / 957, lengths 753 / 752, distances 662 / 661: their code-length codes (the literal and distance codes of tok48 have a depth
  of exactly 15 and are the optimum)"""
import os
import struct
import subprocess
import zlib

import pytest

import dfl_cases as D
from test_bam_core import _build, _run

NAMES = [c.name for c in D.cases()]
TRACE = struct.Struct("<II286s30s19s286I30I19I")


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """every piece of the table through the sanitizer build in one run: (level 0 members, level 1 members, level 1 traces) per case"""
    tmp = tmp_path_factory.mktemp("dfl")
    pieces = [[c.data[p:p + D.PIECE] for p in range(0, len(c.data), D.PIECE)] for c in D.cases()]
    out = {}
    for level in (0, 1):
        fi, fo, ft = (str(tmp / f"{x}{level}.bin") for x in ("cases", "results", "trace"))
        with open(fi, "wb") as f:
            f.write(struct.pack("<I", sum(len(p) for p in pieces)))
            for ps in pieces:
                for pc in ps:
                    f.write(struct.pack("<II", level, len(pc)) + pc)
        exe = _build("deflate_core_host")
        res = _run(exe, fi, fo) if level == 0 else _run_traced(exe, fi, fo, ft)
        p = 0
        for c, ps in zip(D.cases(), pieces):
            ms = []
            for _ in ps:
                n = struct.unpack_from("<I", res, p)[0]; p += 4
                ms.append(res[p:p + n]); p += n
            out.setdefault(c.name, []).append(ms)
        assert p == len(res)
        if level == 1:
            with open(ft, "rb") as f:
                tr = f.read()
            assert len(tr) == TRACE.size * sum(len(p) for p in pieces)
            p = 0
            for c, ps in zip(D.cases(), pieces):
                ts = []
                for _ in ps:
                    v = TRACE.unpack_from(tr, p); p += TRACE.size
                    ts.append(dict(form=v[0], bits=v[1], llen=list(v[2]), dlen=list(v[3]), cllen=list(v[4]), lfreq=list(v[5:291]), dfreq=list(v[291:321]), clfreq=list(v[321:340])))
                out[c.name].append(ts)
    return out


def _run_traced(exe, fi, fo, ft):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:verify_asan_link_order=0")
    r = subprocess.run([exe, fi, fo, ft], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    with open(fo, "rb") as f:
        return f.read()


def check_code(what, hist, lens, limit, name):
    """complete; the Huffman optimum where its depth fits the limit, no less where it does not; returns (cost, optimum) of a limited code"""
    assert len(hist) == len(lens) and all((h > 0) <= (l > 0) for h, l in zip(hist, lens)), (name, what)
    assert max(lens) <= limit and D.kraft(lens, limit) == 1 << limit, (name, what, "complete")
    if sum(h > 0 for h in hist) < 2:                             # place-holders: one-bit codes
        assert sorted(l for l in lens if l) == [1, 1] and lens[0] == 1, (name, what)
        return None
    assert all((h > 0) == (l > 0) for h, l in zip(hist, lens)), (name, what)
    depth, best = D.huff(hist)
    cost = sum(h * l for h, l in zip(hist, lens))
    if depth <= limit:
        assert cost == best, (name, what, cost, best)
        return None
    assert cost >= best and max(lens) == limit, (name, what, cost, best)
    return cost, best


@pytest.mark.parametrize("name", NAMES)
def test_case(core, name):
    from bwamem_hip.lib import bgzf_compress, bgzf_eof, inflate_bgzf
    c = next(c for c in D.cases() if c.name == name)
    san0, san1, trace = core[name]
    pieces = [c.data[p:p + D.PIECE] for p in range(0, len(c.data), D.PIECE)]
    # level 0: the stored form's bytes
    blob0 = bgzf_compress(c.data, 0, host=True)
    assert blob0 == b"".join(san0) == b"".join(D.stored_member(pc) for pc in pieces)
    # level 1: the host entry point and the sanitizer build give the same bytes
    blob = bgzf_compress(c.data, 1, host=True)
    assert blob == b"".join(san1)
    assert bgzf_compress(c.data, 1, host=True) == blob
    assert inflate_bgzf(blob + bgzf_eof(), host=True) == c.data
    r = D.evaluate(c.data, blob)
    for x, pc, t in zip(r.pieces, pieces, trace):
        assert zlib.decompress(x.member, 31) == pc == x.text and x.crc32 == zlib.crc32(pc) and x.isize == len(pc)
        lf, df, _ = D.histograms(x.model)
        assert t["lfreq"] == lf and t["dfreq"] == df, "the counts are the tokens'"
        clhist = [(t["llen"][:max(257, max(i + 1 for i in range(286) if t["llen"][i]))] + t["dlen"][:max([1] + [i + 1 for i in range(30) if t["dlen"][i]])]).count(i) for i in range(16)]
        assert t["clfreq"][:16] == clhist and not any(t["clfreq"][16:]) and not any(t["cllen"][16:])
        limited = [check_code("literal / length", lf, t["llen"], 15, name), check_code("distance", df, t["dlen"], 15, name), check_code("code length", clhist, t["cllen"][:16], 7, name)]
        for what, v in zip(("literal / length", "distance", "code length"), limited):
            if v and len(pieces) == 1:
                print(f"{name}: {what} code limited, cost / optimum {v[0]} / {v[1]}")
        # the estimate is what the block costs, and the smaller form is written (a tie: stored)
        bits = D.dynamic_bits(t["llen"], t["dlen"], t["cllen"], x.model)
        assert t["bits"] == bits, (name, "estimated", t["bits"], "the tokens cost", bits)
        dyn = 18 + (bits + 7) // 8 + 8
        assert x.form == ("dynamic" if dyn < len(pc) + 31 else "stored") and t["form"] == (2 if x.form == "dynamic" else 0), (name, dyn, len(pc) + 31)
        if getattr(c, "kind", None):
            assert dyn == len(pc) + (30 if c.kind == "smaller" else 31), (name, dyn)
        if x.form == "dynamic":
            assert [tok[2] for tok in x.tokens] == x.model, "the model's tokens"
            assert x.end - 144 == bits and len(x.member) == dyn
            assert x.llen == t["llen"][:x.nlen] and x.dlen == t["dlen"][:x.ndist] and x.cllen == t["cllen"]
            assert x.eob[1] == x.llen[256]
        else:
            assert x.member == D.stored_member(pc)
    bad = [k for k, v in c.must.items() if not v(r)]
    assert not bad, (name, bad)


def test_the_table_names_its_reach():
    """what the table must reach, by the names of its musts (a builder that loses one fails test_case; a table that loses one fails here)"""
    musts = " | ".join(k for c in D.cases() for k in c.must)
    for want in ("deeper than 15 bits", "deeper than 7 bits", "(offset mod 32) + bits > 64", "a token of 48 bits", "every length symbol", "every distance symbol", "32 769 is refused",
                 "a carry of exactly 64", "a carry of 65", "four steps", "skipped step", "last byte", "position", "two pieces", "one hash", "latest wins", "ncode 12", "ncode: 19",
                 "n + 30 bytes", "stored", "every alignment"):
        assert want in musts, want
