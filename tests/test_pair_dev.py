"""The pairing stage without a GPU: the host walk (bmh_finalize_pairs, no mate rescue) against the plain restatement of tests/pair_cases.py on hand-made
regions that force the branches simulated reads reach by chance -- and the proof that the generated sets do reach them.  The device kernel is compared with
the same host records in tests/test_pair_dev_gpu.py."""
import numpy as np
import pytest

import pair_cases as pc


@pytest.mark.parametrize("name", list(pc.CONFIGS))
def test_host_walk_equals_the_restatement(name):
    g = pc.case(name)
    assert len(g.fin) == len(g.regs) and np.array_equal(g.per_read, g.rpr)           # nothing was merged or dropped
    want_failed = [1, 0, 0, 1] if name == "two_orient" else [1, 0, 1, 1]
    assert g.pes[:, 2].astype(int).tolist() == want_failed, g.pes
    assert 130 <= g.pes[1, 0] <= 165 and 435 <= g.pes[1, 1] <= 470 and abs(g.pes[1, 3] - 300) < 3 and abs(g.pes[1, 4] - 30) < 2.5, g.pes[1]
    if name == "two_orient":
        assert abs(g.pes[2, 3] - 500) < 8 and abs(g.pes[2, 4] - 40) < 6, g.pes[2]
    a = g.opt.ep.a
    n_paired = 0
    for p in range(g.n_pairs):
        R = g.res[p]
        what = (name, p, g.intent[p], sorted(g.labels[p]))
        for r in (0, 1):
            rd = 2 * p + r
            recs = g.fin[g.off[rd]:g.off[rd + 1]]
            assert int(g.h_rec[rd]) == R.z[r], what                    # the record the mate's fields are taken from
            rep = recs[(recs[:, 15] & 1) != 0]
            flags = rep[:, 14] if len(rep) else np.array([g.unflag[rd]])
            assert len(rep) or g.unflag[rd], what
            assert all(bool(f & 2) == R.proper and f & 1 and f & (0x40 << r) for f in flags), what
            if R.paired:
                c = recs[R.z[r]]
                assert c[15] & 1 and c[13] <= pc.raw_mapq(int(c[1]), a), what
                assert (recs[:, 15] & 1).sum() == 1 + (name == "alt" and R.n[r] > R.n_pri[r] and bool(recs[R.n_pri[r], 15] & 1)), what
        n_paired += R.paired
    assert n_paired == 0 if name == "no_pairing" else n_paired > 1200


@pytest.mark.parametrize("name", ["default", "two_orient"])
def test_generated_pairs_take_every_branch(name):
    g = pc.case(name)
    cnt = pc.class_counts(g)
    assert g.n_pairs % 64
    for k in ("a", "b", "c", "d", "e", "f", "g", "h", "h_inside", "i", "k"):
        assert cnt.get(k, 0) >= 30, (k, cnt)
    assert cnt["j63"] + cnt["j64"] + cnt["j65"] >= 30 and min(cnt["j63"], cnt["j64"], cnt["j65"]) >= 8, cnt
    assert cnt["l_in"] >= 12 and cnt["l_out"] >= 12, cnt                # inserts low, high / low - 1, high + 1
    for k in ("g_ctg", "g_far", "g_ff", "g_none1", "g_none2", "g_lowT3", "lowT_chosen"):
        assert cnt.get(k, 0) >= 8, (k, cnt)
    assert cnt["g_position"] >= 30 and cnt["d_both"] >= 10, cnt
    assert sum(max(g.res[p].z) > 0 for p in range(g.n_pairs) if g.res[p].paired) >= 20
    assert sum(g.res[p].n_sub >= 2 for p in range(g.n_pairs)) >= 20
    assert cnt["n_sub1"] >= 30 and cnt["n_sub2"] >= 10 and cnt["n_sub3"] >= 10, cnt
    assert cnt["sub_edge_in"] >= 5 and cnt["sub_edge_out"] >= 5, cnt    # a runner-up exactly at, and one just beyond, the window below the second best
    assert {float(x) for x in np.unique(g.frac)} == {0.0, float(np.float32(0.3)), float(np.float32(0.9))}
    # class j's split of the hits between the reads
    splits = {tuple(g.res[p].n) for p in range(g.n_pairs) if sum(g.res[p].n) in (63, 64, 65)}
    assert {(1, 63), (32, 32)} <= splits | {(b, a_) for a_, b in splits}, splits
    # equal candidates are really decided by the hash: both outcomes occur
    zc = {tuple(g.res[p].z) for p in range(g.n_pairs) if "c" in g.labels[p]}
    assert len(zc) >= 2, zc


def test_alt_configuration_reaches_the_alt_branches():
    g = pc.case("alt")
    cnt = pc.class_counts(g)
    assert cnt["alt_hit"] >= 200 and cnt["a"] >= 30 and cnt["d"] >= 30 and cnt["e"] >= 30 and cnt["g"] >= 30, cnt
    supp = low_pri = 0
    for p in range(g.n_pairs):
        R = g.res[p]
        for r in (0, 1):
            if R.n[r] > R.n_pri[r]:
                recs = g.fin[g.off[2 * p + r]:g.off[2 * p + r + 1]]
                supp += bool(R.paired and recs[R.n_pri[r], 14] & 0x800)                       # the best ALT hit as a supplementary record of a paired read
                low_pri += bool(not R.paired and R.n_pri[r] and R.z[r] == R.n_pri[r])          # the hit of the primary assembly below T: the ALT hit is shown to the mate
    assert supp >= 30 and low_pri >= 8, (supp, low_pri)


@pytest.mark.parametrize("name", list(pc.CONFIGS))
def test_no_pair_score_is_close_to_an_integer(name):
    """The device hands a pair back when a score falls within 1e-6 of an integer before it is truncated; the GPU test demands that none is handed
    back, so the generated sets keep a margin of 1e-4 (the device's erfc / log differ from libm's in the last bits).  A seed that breaks this is changed."""
    g = pc.case(name)
    worst = min((abs(c[1] - round(c[1])) for R in g.res for c in R.cands), default=1.0)
    assert worst > 1e-4, worst


def test_host_walk_under_sanitizers(tmp_path):
    """bmh_finalize_pairs on the ALT configuration in a stand-alone program (tests/pair_post_host.cpp) built with -fsanitize=address,undefined: the same records
    as in this process, and nothing for the sanitizers to report."""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "bwa-mem_gpu_amd", "csrc")
    cxx = "/opt/rocm/llvm/bin/clang++"                                # the host sources include HIP's headers: the host side alone, no device code, no HIP runtime linked
    if not os.path.exists(cxx):
        pytest.skip("no HIP compiler to build the host sources with")
    out = os.path.join(here, "_build", "pair_post_host.d"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "pair_post_host")
    src = [os.path.join(here, "pair_post_host.cpp")] + [os.path.join(csrc, f) for f in ("pair_post.cpp", "regs_post.cpp", "local_sw.cpp")]
    dep = src + [os.path.join(csrc, f) for f in ("regs_post.h", "bmh_internal.h", "pair_kernels.h", "klib_sort.h", "local_sw.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in dep):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
        subprocess.check_call([cxx, "-x", "hip", "--offload-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-c"] + san + src, cwd=out)
        subprocess.check_call([cxx] + san + [os.path.splitext(os.path.basename(f))[0] + ".o" for f in src] + ["-o", exe], cwd=out)
    g = pc.case("alt")
    fi, fo = str(tmp_path / "pairs_case.bin"), str(tmp_path / "pairs_result.bin")
    pc.dump_case(g, fi)
    r = subprocess.run([exe, fi, fo], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the program) reported:\n" + err[-4000:]
    fin, opr, h, uf, pes = pc.load_result(fo, g.n_reads)
    assert np.array_equal(fin, g.fin) and np.array_equal(opr, g.per_read) and np.array_equal(h, g.h_rec) and np.array_equal(uf, g.unflag) and np.array_equal(pes, g.pes)
