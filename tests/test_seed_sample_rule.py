"""Which occurrences of an SMEM chaining reads: mem_chain's loop (src/bwamem.c:430-436) against the closed form the device uses -- chain_core.h
(step, n_it) when it reads them and expand_locate_kernel (csrc/seed_kernels.hip: sample_rule) when a sampled batch writes only those."""
import pytest


def mem_chain_slots(s: int, max_occ: int) -> list:
    """the loop as mem_chain runs it: step = s > max_occ ? s / max_occ : 1; for (k = count = 0; k < s && count < max_occ; k += step, ++count)"""
    step = s // max_occ if s > max_occ else 1
    out, k, count = [], 0, 0
    while k < s and count < max_occ:
        out.append(k)
        k += step
        count += 1
    return out


def sample_rule(s: int, max_occ: int):
    """(step, n_it) of sample_rule in csrc/seed_kernels.hip: slot j * step for j < n_it"""
    step, n_it = 1, s
    if s > max_occ:
        step = s // max_occ
        n_it = min((s + step - 1) // step, max_occ)
    return step, n_it


def sampled_slots(s: int, max_occ: int) -> list:
    """the slots of a group of s that a batch sampled with max_occ holds (max_occ 0: all of them)"""
    if max_occ == 0:
        return list(range(s))
    step, n_it = sample_rule(s, max_occ)
    return [j * step for j in range(n_it)]


@pytest.mark.parametrize("max_occ", [1, 2, 3, 5, 500])
def test_closed_form_is_mem_chains_loop(max_occ):
    for s in range(1, 4001):
        step, n_it = sample_rule(s, max_occ)
        want = mem_chain_slots(s, max_occ)
        assert [j * step for j in range(n_it)] == want, (s, max_occ)
        assert n_it == len(want) <= max_occ and want[-1] < s
        # chain_core.h computes n_it by the same expression for every s, also s <= max_occ (step 1)
        assert n_it == min((s + step - 1) // step, max_occ)
        if s <= max_occ:
            assert want == list(range(s))
