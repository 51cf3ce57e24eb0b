"""CPU checks of the case builder the batched-MSM GPU tests draw from (tests/msm_batch_cases.py): no GPU.  The closed form the builder
attaches to every vector kind equals the oracle's literal bucket_msm over the same points, and every call list keeps the conditions the
GPU tests rely on (distinct vectors, a TOP / ONE neighbour pair, a Z vector and an empty polynomial in the middle of a batch, every kind
and every length somewhere, one call that leaves member 1 without work, one with the longest vector last behind a length-1 vector)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import bigint_model as M
from tests import msm_batch_cases as B


def _points(n, a, d):
    proj = np.zeros((n, 18), dtype=np.uint64)
    proj[:, :12] = O.points_progression(n, a, d)[:, :12]
    proj[:, 12:] = O.fp_one()
    return proj


@pytest.mark.parametrize("m", [1, 5, 65, 150])
def test_closed_form_of_every_kind_is_the_oracles_bucket_msm(m):
    """2 m <= 300 points: for every call of the builder, every vector's closed form (from the kind's parameters) names the group element
    the oracle's bucket_msm (src/msm.rs:76-118) computes from the ARRAY over the same points, scalars past the SRS dropped"""
    a, d = B.progression(0, m)
    proj = _points(2 * m, a, d)
    gen = _points(1, 1, 0)                                               # the generator: k G by the oracle, and by Python integers once per call
    seen = set()
    for k in B.KS:
        for j, v in enumerate(B.build_call(k, m, a, d, 0x77 + k, radix=(B.RADIX[21], 13) if m == 150 else None)):
            seen.add(v.kind)
            used = min(v.n, 2 * m)
            assert v.arr.shape == (v.n, 4) and v.arr.dtype == np.uint64
            want = bytes(O.g1_bytes96(O.bucket_msm(gen, O.fr_from_int(v.k).reshape(1, 4))))
            if j == len(B.CALL_SPECS[k]) - 1:
                assert want == M.enc96(M.ec_mul(v.k))
            if used == 0:
                assert v.k == 0
                continue
            assert bytes(O.g1_bytes96(O.bucket_msm(proj[:used], v.arr[:used]))) == want, (m, k, j, v.kind, v.lname)
    assert seen == set(B.KINDS)


def test_radix_edge_scalars_reach_a_vector_of_every_call():
    """the boundary scalars of radix R sit in one U vector of a call (where one is long enough) and the closed form follows them"""
    m, (a, d) = 150, B.progression(0, 150)
    edges = B.radix_edge_scalars(B.RADIX[21], 13)
    assert {B.RADIX[21] // 2, B.RADIX[21] // 2 - 1, B.RADIX[21] // 2 + 1, (B.RADIX[21] ** 5 + 1) % B.Q} <= set(edges)
    for k in (4, 8, 9):
        vecs = B.build_call(k, m, a, d, 0x99, radix=(B.RADIX[21], 13))
        plain = B.build_call(k, m, a, d, 0x99)
        patched = [j for j, (u, v) in enumerate(zip(vecs, plain)) if u.kind != "DUP" and not (u.arr == v.arr).all()]
        assert len(patched) == 1 and vecs[patched[0]].kind == "U" and vecs[patched[0]].seed is None
        got = set(O.fr_array_to_ints(vecs[patched[0]].arr))
        assert set(edges) <= got


@pytest.mark.parametrize("c,m,paths", B.SHAPES, ids=["c%d-m%d" % (c, m) for c, m, _ in B.SHAPES])
def test_every_call_list_keeps_its_conditions(c, m, paths):
    a, d = B.progression(c, m)
    radix = (B.RADIX[c], paths[max(paths)]["W"]) if c in B.RADIX else None
    calls = {k: B.build_call(k, m, a, d, B.shape_seed(c, m) + k, radix) for k in B.KS}
    assert sorted(calls) == [2, 3, 4, 5, 8, 9] and all(len(v) == k for k, v in calls.items())
    for k, vecs in calls.items():
        B.check_call(vecs, m)
    assert set(paths) <= set(calls)
    for J in paths:                                                       # the path is asserted after a call of J full-length vectors
        assert max(v.n for v in calls[J]) >= m, J                          # (the plan takes the longest vector's length for all J)
    every = [v for vecs in calls.values() for v in vecs]
    assert {v.kind for v in every} == set(B.KINDS) and {v.lname for v in every} == set(B.LENGTHS)
    assert any(B.has_top_one_pair(v, m) for v in calls.values())
    assert any(B.has_zero_and_empty_in_the_middle(v) for v in calls.values())
    assert any(v[0].n == 1 and v[-1].n == max(u.n for u in v) == 2 * m + 9 for v in calls.values())      # longest last, length 1 first
    assert any(all(u.n <= m for u in v) and any(u.n == m for u in v) for v in calls.values())            # member 1 gets nothing
    if radix:
        assert any(u.kind == "U" and u.seed is None for v in calls.values() for u in v)
