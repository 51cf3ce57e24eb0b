"""-m gpu: the J-vector MSM pipeline (msm_launch_many with J > 1: one sort keyed (vector, bucket), one accumulation, one fix-up, one tree over
J * 2^(c-1) buckets, J Horner passes) at every edge it has of its own.  The vehicle is what ships: bp_commit_many_device on a group context
(the COMMIT_GROUP_BATCH route of commit_many), here a rehearsal group of two members on device 0 with m points each, over an SRS of 2 m points
P_i = (a + i d) G with fixed-base tables of a chosen width.  Every commitment is held by itself against the closed form
(sum_i s_i (a + i d)) G in Python integers -- never against the library -- and against bp_commit_device of the same polynomial, bytes for
bytes; every shape asserts the path the library reports for it (Context.msm_path), so a retune that moves a shape off the branch it was
chosen for fails here by name.  Vector kinds, lengths and call lists: tests/msm_batch_cases.py (checked on the CPU by
tests/test_msm_batch_cases.py)."""
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from oracle import oracle as O
from tests import bigint_model as M
from tests import msm_batch_cases as B
from tests.gpu_common import Q, oracle_dot, progression_bytes

pytestmark = pytest.mark.gpu
PATH_KEYS = ("J", "c", "W", "radix", "sort", "pb", "packed", "flat", "wide8", "fixup", "n_wide")


def pick(path):
    return {k: path[k] for k in PATH_KEYS}


@pytest.fixture(scope="module")
def group():
    ctx = bp.Context([0, 0])
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def single():
    ctx = bp.Context(0)
    yield ctx
    ctx.close()


class Srs:
    """one SRS with tables per (context, shape), kept while consecutive cases use it"""

    def __init__(self):
        self.key, self.ctx, self.h = None, None, None

    def get(self, ctx, c, m):
        if self.key != (id(ctx), c, m):
            self.drop()
            a, d = B.progression(c, m)
            self.h = ctx.srs_generate_progression(2 * m, a, d)
            info = ctx.srs_precompute(self.h, c)
            assert info["window_bits"] == c
            self.key, self.ctx = (id(ctx), c, m), ctx
        return bp.Setup(self.h, ctx, tables=False)       # (tables=False: the tables of width c are already there)

    def drop(self):
        if self.h is not None:
            self.ctx.srs_free(self.h)
        self.key, self.ctx, self.h = None, None, None


@pytest.fixture(scope="module")
def srs(group, single):               # (after the contexts, so that it is torn down before them)
    s = Srs()
    yield s
    s.drop()


def device_polys(ctx, vecs, on_device):
    """the call's polynomials in HBM; on_device: U vectors that kept their seed are generated there (the same SplitMix64 stream)"""
    import torch
    polys = []
    for v in vecs:
        if on_device and v.kind == "U" and v.seed is not None and v.n:
            t = torch.empty((v.n, 4), dtype=torch.int64, device=torch.device("cuda", ctx.device))
            ctx.synthetic_scalars_device(t.data_ptr(), v.n, v.seed)
            assert (t[:100].cpu().numpy().view(np.uint64) == v.arr[:100]).all() and (t[-1:].cpu().numpy().view(np.uint64) == v.arr[-1:]).all()
            polys.append(bp.DevicePolynomial(t, bp.BASIS_MONOMIAL, ctx))
        else:
            polys.append(bp.DevicePolynomial(v.arr, bp.BASIS_MONOMIAL, ctx))
    return polys


def check_call(ctx, setup, vecs, a, d, N, where):
    """commit_many_device of the call: every result against the closed form by itself, and against commit_device of the same polynomial"""
    polys = device_polys(ctx, vecs, on_device=N // 2 >= B.DEVICE_GENERATED_FROM)
    got = bp.commit_many_device(setup, polys)
    assert len(got) == len(vecs)
    for j, (v, p) in enumerate(zip(vecs, polys)):
        k = oracle_dot(v.arr[:N], a, d) if min(v.n, N) else 0
        assert k == v.k, (where, j, v.kind, v.lname)                      # the kind's closed form and the array agree
        assert got[j] == M.enc96(M.ec_mul(k)), (where, j, v.kind, v.lname)
    path = ctx.msm_path(0)                                               # (before the single commitments below launch their own)
    for j, p in enumerate(polys):
        assert bp.commit_device(setup, p) == got[j], (where, j, "commit_device")
    return path


def radix_of(c, paths):
    return (B.RADIX[c], paths[max(paths)]["W"]) if c in B.RADIX else None


SHAPE_IDS = ["c%d-m%d" % (c, m) for c, m, _ in B.SHAPES]


@pytest.mark.parametrize("k", B.KS)
@pytest.mark.parametrize("c,m,paths", B.SHAPES, ids=SHAPE_IDS)
def test_batched_commit_closed_form_and_path(group, srs, c, m, paths, k):
    """two members of m points, tables of width c, the call of k vectors (batches of up to four): closed form, commit_device, and -- after a
    call whose last batch has J vectors with the longest on all of member 0's points -- the path of member 0 for that J"""
    a, d = B.progression(c, m)
    setup = srs.get(group, c, m)
    assert group.n_shards() == 2
    vecs = B.build_call(k, m, a, d, B.shape_seed(c, m) + k, radix_of(c, paths))
    path = check_call(group, setup, vecs, a, d, 2 * m, (c, m, k))
    print("path c=%d m=%d k=%d: %s" % (c, m, k, path))
    last = vecs[(k - 1) // B.BATCH * B.BATCH:]
    assert max(v.n for v in last) >= m or k == 5                         # member 0's longest slice is m (k = 5 ends on a length-1 vector)
    assert path["J"] == len(last) and path["c"] == c
    # the whole path is pinned only by the calls whose last batch has a J of the shape's row (a J = 2 or J = 3 row: one call of the six);
    # the other calls check J and c alone
    if len(last) in paths and k != 5:
        assert pick(path) == paths[len(last)], (c, m, k)


@pytest.mark.parametrize("c,m,paths", [s for s in B.SHAPES if s[0] in (8, 17)], ids=["c8-m300", "c17-m20000"])
def test_the_same_calls_on_a_single_device(single, srs, c, m, paths):
    """bp.Context(0): the same calls take concurrent lanes in rounds of three (8 -> 3+3+2, 4 -> 3+1), one vector per pipeline: same closed
    forms, and the path says J == 1"""
    a, d = B.progression(c, m)
    setup = srs.get(single, c, m)
    for k in B.KS:
        vecs = B.build_call(k, m, a, d, B.shape_seed(c, m) + k)
        path = check_call(single, setup, vecs, a, d, 2 * m, ("single", c, m, k))
        assert path["J"] == 1, (c, m, k, path)
        assert single.msm_path()["J"] == 1


def test_three_members_and_their_seams():
    """Context([0, 0, 0]) over 1000 points: shards of 334, 333 and 333 (asserted from the library's own reports), c = 6, eleven polynomials
    whose lengths end before, on and after each seam: batches of 4 + 4 + 3"""
    N, c = 1000, 6
    rnd = random.Random(0x3333)
    a, d = rnd.randrange(1, Q), rnd.randrange(1, Q)
    many = bp.Context([0, 0, 0])
    raw = progression_bytes(N, a, d)
    h = many.srs_generate_progression(N, a, d)
    assert many.n_shards() == 3 and many.srs_len(h) == N
    seams = [334, 667]
    for s in seams:                                   # the range entry points up to, from and across each seam name the progression's points
        for first, cnt in ((s - 1, 1), (s, 1), (s - 1, 2), (s, 0), (s - 334 + 1, 333)):
            assert many.srs_export(h, first, cnt) == raw[96 * first: 96 * (first + cnt)], (first, cnt)
            assert many.srs_check_subgroup(h, first, cnt) is None
    assert many.srs_precompute(h, c)["window_bits"] == c
    ones = np.tile(bp.scalar_from_int(1), (N, 1))     # one non-zero digit per scalar: a member's additions are its points
    assert many.msm(h, ones) == M.enc96(M.ec_mul((N * a + d * (N * (N - 1) // 2)) % Q))
    assert [s["mixed_adds"] for s in many.msm_member_stats()] == [334, 333, 333]
    setup = bp.Setup(h, many, tables=False)
    lens = [0, 1, 333, 334, 335, 666, 667, 668, 999, 1000, 1009]
    kinds = ["U", "U", "TOP", "ONE", "EQ", "U", "HOT", "SMALL", "TOP", "ONE", "U"]
    vecs = []
    for j, (n, kind) in enumerate(zip(lens, kinds)):
        used = min(n, N)
        if kind == "U":
            arr = O.splitmix_scalars(n, 0x3300 + j) if n else np.zeros((0, 4), dtype=np.uint64)
        elif kind == "HOT":
            arr = np.zeros((n, 4), dtype=np.uint64)
            arr[666] = bp.scalar_from_int(rnd.randrange(2, Q))           # the last point of member 1
        elif kind == "SMALL":
            arr = bp.scalars_from_ints([(i * 7919 + 5) % 65536 for i in range(n)])
        else:
            arr = np.tile(bp.scalar_from_int({"TOP": Q - 1, "ONE": 1}.get(kind) or rnd.randrange(2, Q)), (n, 1))
        vecs.append(arr)
    polys = [bp.DevicePolynomial(v, bp.BASIS_MONOMIAL, many) for v in vecs]
    got = bp.commit_many_device(setup, polys)
    want = [M.enc96(M.ec_mul(oracle_dot(v[:N], a, d) if len(v) else 0)) for v in vecs]
    assert got == want and len(set(want[1:])) == 10
    for r, J in enumerate((3, 3, 3)):                 # the last batch: lengths 999, 1000, 1009 reach every member
        assert many.msm_path(r)["J"] == J and many.msm_path(r)["c"] == c
    assert [bp.commit_device(setup, p) for p in polys] == want
    with pytest.raises(bp.BpError):
        many.msm_path(3)
    many.close()


def test_the_retreat_to_one_by_one():
    """A batch too long for the partition sort would be refused (BP_ERR_TOO_LARGE inside the library): commit_many asks the plan of every round
    before it launches anything (csrc/commit_plan.hpp; the same edge without a GPU: tests/test_commit_plan.py) and goes one commitment at a time.
    c = 16, W = 16, J = 4: kb = 17; pb reaches 13 from 12 288 * 2^13 entries on, and the rule that keeps pb at PART_MAX_BITS = 12 holds
    while entries >> 12 <= 32 768, i.e. below 32 769 * 4 096 = 2^27 + 4 096 = 134 221 824 entries = W * n * J = 64 n: refused from
    n = 2 097 216 points per member (the packed rule does not apply: kb + vb = 17 + 27 = 44 <= 32 + 13).  Refused at the first batch, and at
    a later batch while the first one fits; the context works for a small batch afterwards."""
    import torch
    m, c = 2097216, 16
    ctx = bp.Context([0, 0])
    rnd = random.Random(0x2E72)
    a, d = rnd.randrange(1, Q), rnd.randrange(1, Q)
    h = ctx.srs_generate_progression(2 * m, a, d)
    assert ctx.srs_precompute(h, c) == {"window_bits": 16, "windows": 16, "bytes": 16 * 2 * m * 128}
    setup = bp.Setup(h, ctx, tables=False)
    t = torch.empty((4, 2 * m, 4), dtype=torch.int64, device="cuda")
    host, want = [], []
    for j in range(4):
        ctx.synthetic_scalars_device(t[j].data_ptr(), 2 * m, 0x2E7200 + j)
        sc = O.splitmix_scalars(2 * m, 0x2E7200 + j)
        assert (t[j, :50].cpu().numpy().view(np.uint64) == sc[:50]).all()
        host.append(sc)
        want.append(M.enc96(M.ec_mul(O.dot_progression(sc, a, d))))
    assert len(set(want)) == 4
    full = [bp.DevicePolynomial(t[j], bp.BASIS_MONOMIAL, ctx) for j in range(4)]
    short = [bp.DevicePolynomial(host[j][:1000].copy(), bp.BASIS_MONOMIAL, ctx) for j in range(4)]
    want_short = [M.enc96(M.ec_mul(oracle_dot(host[j][:1000], a, d))) for j in range(4)]
    # below the bound at the same m: three full vectors are 48 n entries and run as one batch
    assert bp.commit_many_device(setup, full[:3]) == want[:3] and ctx.msm_path(0)["J"] == 3 and ctx.msm_path(1)["J"] == 3
    # 1. refused at the first batch
    assert bp.commit_many_device(setup, full) == want
    assert ctx.msm_path(0)["J"] == 1 and ctx.msm_path(0)["c"] == 16
    # a small batch in between: the next call starts from a context that last ran J = 4
    assert bp.commit_many_device(setup, short) == want_short and ctx.msm_path(0)["J"] == 4
    # 2. the first batch fits, the second would be refused: everything goes one by one
    assert bp.commit_many_device(setup, short + full) == want_short + want
    assert ctx.msm_path(0)["J"] == 1
    # the context is usable for a batch afterwards
    assert bp.commit_many_device(setup, short) == want_short
    assert pick(ctx.msm_path(0)) == {"J": 4, "c": 16, "W": 16, "radix": 0, "sort": 2, "pb": 11, "packed": 1, "flat": 1, "wide8": 0, "fixup": 1,
                                      "n_wide": 4}         # (pb = 11: the table index spans 16 rows of m points, 26 bits: packed by raising pb)
    ctx.srs_free(h)
    ctx.close()


# (c, n) of test_table_width_sweep_on_the_shipped_library (c <= 16), test_windows_wider_than_16_bits (c >= 17) and
# test_north_star_shard_2p21_auto_width (the last): what the single-vector pipeline reports for them.  Between them: both fix-up forms,
# packed 0 / 1, flat 0 / 1, wide8, n_wide 0 and >= 2 (sort == 1 is asserted where the 2^24 MSM already runs:
# test_full_size_2p24_closed_form_both_paths).  Every row: J = 1, sort = 2 (partition).
SINGLE_PATHS = [
    # c, n, W, radix, pb, packed, flat, wide8, fixup, n_wide
    (4, 1 << 10, 64, 0, 2, 1, 0, 0, 0, 0),
    (8, 1 << 12, 32, 0, 3, 1, 0, 0, 0, 0),
    (12, 1 << 16, 22, 0, 6, 1, 0, 0, 0, 0),
    (16, 1 << 18, 16, 0, 8, 1, 0, 0, 0, 0),
    (17, (1 << 14) + 13, 16, 0, 4, 1, 0, 0, 1, 3),
    (19, (1 << 16) + 13, 14, 0, 7, 1, 0, 0, 1, 6),
    (20, (1 << 17) + 13, 13, 0, 9, 1, 0, 0, 1, 7),
    (21, (1 << 18) + 13, 13, B.RADIX[21], 11, 1, 1, 0, 1, 8),
    (22, (1 << 19) + 13, 12, B.RADIX[22], 9, 0, 0, 1, 1, 9),
    (20, 1 << 21, 13, 0, 11, 0, 0, 1, 1, 7),
]


@pytest.mark.parametrize("row", SINGLE_PATHS, ids=["c%d-n%d" % r[:2] for r in SINGLE_PATHS])
def test_paths_of_the_single_vector_shapes(single, row):
    """the paths the width sweep's docstring says its shapes select, as the library reports them: one uniform MSM through the tables against
    the closed form, then the report"""
    import torch
    c, n, W, radix, pb, packed, flat, wide8, fixup, n_wide = row
    rnd = random.Random(0x9A7 + c)
    a, d = rnd.randrange(1, Q), rnd.randrange(1, Q)
    h = single.srs_generate_progression(n, a, d)
    assert single.srs_precompute(h, c) == {"window_bits": c, "windows": W, "bytes": W * n * 128}
    t = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    single.synthetic_scalars_device(t.data_ptr(), n, 0x9A700 + c)
    sc = O.splitmix_scalars(n, 0x9A700 + c)
    want = M.enc96(M.ec_mul(oracle_dot(sc, a, d)))
    assert bp.sum_partials(single.msm_partial(h, None, device_ptr=t.data_ptr(), n=n)) == want and single.msm_stats()["tables"]
    path = single.msm_path()
    print("path c=%d n=%d: %s" % (c, n, path))
    assert pick(path) == {"J": 1, "c": c, "W": W, "radix": radix, "sort": 2, "pb": pb, "packed": packed, "flat": flat, "wide8": wide8,
                          "fixup": fixup, "n_wide": n_wide}
    assert path["chunk"] >= 4
    single.srs_free(h)
