"""Host checks of the attention launch plan: every form ``sgp_attention_plan`` can return is reached by a listed kernel
case on each side of each boundary it decides on, and sizes outside the domain return ``SGP_EUNSUP`` with the reason."""
import ctypes

import pytest

import attention_forms as AF
from sgp_amd import hip


def _plan(c):
    return hip.attention_plan(c.L, c.d, c.heads, c.n_seq, c.causal, c.q_first)


def test_every_form_is_reached_on_both_sides_of_its_boundaries():
    by_d = {}
    for c in AF.CASES:
        by_d.setdefault(c.d, set()).add(_plan(c)["form"])
    assert all(len(v) == 1 for v in by_d.values())
    forms = {d: next(iter(v)) for d, v in by_d.items()}
    assert set(forms.values()) == set(hip.ATTENTION_FORMS)
    # the plan's form as a function of d over the whole domain: the boundaries found by scanning, each with a listed case on either side
    scan = {d: hip.attention_plan(17, d, 1, 1)["form"] for d in range(8, 129, 8)}
    edges = [(d - 8, d) for d in range(16, 129, 8) if scan[d] != scan[d - 8]]
    assert edges == [(16, 24), (32, 40), (64, 72)]
    for lo, hi in edges:
        assert lo in forms and hi in forms and forms[lo] == scan[lo] and forms[hi] == scan[hi], (lo, hi)
    assert 8 in forms and 128 in forms                              # the ends of the domain


def test_tile_counts_and_grids():
    seen_q, seen_k = set(), set()
    for c in AF.CASES:
        p = _plan(c)
        assert p["dtiles"] == (c.d + 15) // 16 and p["dtiles"] <= p["form"]
        assert p["ktiles"] == (c.L + 15) // 16
        assert p["qtiles"] == (c.L - c.q_first + 15) // 16
        assert p["grid_q"] == -(-c.n_seq * c.heads * p["qtiles"] // p["waves"])
        assert p["grid_k"] == -(-c.n_seq * c.heads * p["ktiles"] // p["waves"])
        seen_q.add(min(p["qtiles"], 3))
        seen_k.add((min(p["ktiles"], 3), c.L % 16 == 0))
    assert seen_q == {1, 2, 3}                                        # one tile, two, many
    assert {k for k, _ in seen_k} == {1, 2, 3}
    assert (1, True) in seen_k and (1, False) in seen_k               # a full and a partial last tile
    lasts = [c for c in AF.CASES if c.last]
    assert lasts and all(_plan(c)["qtiles"] == 1 for c in lasts)
    assert {c.layout for c in AF.CASES} == {"steps", "nodes"} and {c.causal for c in AF.CASES} == {0, 1}
    # a workgroup of partly idle waves and one of exactly full ones
    rem = {c.n_seq * c.heads * _plan(c)["qtiles"] % _plan(c)["waves"] for c in AF.CASES}
    assert 0 in rem and len(rem) > 1


def test_sizes_of_the_issue_are_listed():
    assert {c.L for c in AF.CASES} >= {1, 2, 15, 16, 17, 33, 100, 130, 207, 1040}
    assert {c.d for c in AF.CASES} >= {8, 24, 32, 128}
    assert {c.heads for c in AF.CASES} == {1, 3} and {c.n_seq for c in AF.CASES} == {1, 3, 65}
    assert all(c.heads * c.d <= 256 for c in AF.CASES)
    assert len({c.id for c in AF.CASES}) == len(AF.CASES)


@pytest.mark.parametrize("args,word", AF.OUTSIDE)
def test_outside_the_domain(args, word):
    plan = (ctypes.c_int32 * 8)()
    lib = hip.load()
    assert lib.sgp_attention_plan(*args, plan) == hip.SGP_EUNSUP
    assert word in lib.sgp_last_error().decode()
    with pytest.raises(NotImplementedError, match=word.replace("^", r"\^")):
        hip.attention_require(*args)
    # the entries refuse the same sizes before they look at a pointer
    L, d, heads, n_seq, causal, q_first = args
    assert lib.sgp_attention_fwd_f32(None, 0, None, 0, None, 0, None, 0, None, L, d, heads, n_seq, 1, 0, 0, 1, causal,
                                     q_first, None) == hip.SGP_EUNSUP
    assert lib.sgp_attention_bwd_f32(None, 0, None, 0, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, 0, None, 0,
                                     L, d, heads, n_seq, 1, 0, 0, 1, causal, q_first, None) == hip.SGP_EUNSUP


def test_in_domain_null_pointers_are_einval():
    lib = hip.load()
    assert lib.sgp_attention_plan(12, 8, 1, 3, 0, 0, None) == hip.SGP_EINVAL
    assert lib.sgp_attention_fwd_f32(None, 0, None, 0, None, 0, None, 0, None, 12, 8, 1, 3, 1, 0, 0, 1, 0, 0,
                                     None) == hip.SGP_EINVAL
    assert lib.sgp_attention_workspace_bytes(12, 2, 3) == 12 * 2 * 3 * 4
    assert lib.sgp_attention_workspace_bytes(0, 2, 3) == -1
