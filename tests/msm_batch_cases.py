"""Case builder of the batched-MSM tests (tests/test_gpu_msm_batch.py on the GPU, tests/test_msm_batch_cases.py on the CPU): the vector
kinds, the length lists and the call lists of a commit_many over a group of two members with m points each (SRS of 2 m points,
P_i = (a + i d) G).  Every vector comes with its closed form k = sum_i s_i (a + i d) mod q worked out from the KIND's parameters in Python
integers (never from the array), so a test can hold the array, the closed form and the oracle against each other.

A call is a list of Vec.  Within a call the non-empty, non-zero vectors have pairwise different closed forms unless one is a DUP of the
other, so a result delivered at the wrong place fails."""
import random

import numpy as np

from oracle import oracle as O
from tests import bigint_model as M

Q = M.Q
KINDS = ("U", "Z", "ONE", "TOP", "EQ", "HOT", "SMALL", "DUP")
LENGTHS = ("0", "1", "m-1", "m", "m+1", "2m-1", "2m", "2m+9")
BATCH = 4                       # MSM_MAX_BATCH: vectors in one pipeline


def length_of(name, m):
    return {"0": 0, "1": 1, "m-1": m - 1, "m": m, "m+1": m + 1, "2m-1": 2 * m - 1, "2m": 2 * m, "2m+9": 2 * m + 9}[name]


def _mont(vals):
    return np.array([O.fr_from_int(v) for v in vals], dtype=np.uint64).reshape(-1, 4)


def _sum_points(n, a, d):
    return (n * a + d * (n * (n - 1) // 2)) % Q


class Vec:
    """one scalar vector of a call: kind, length name, length, Montgomery limbs [n, 4], closed form k over the first min(n, N) points,
    seed (U without edge scalars: the array is O.splitmix_scalars(n, seed), which the library can also generate in HBM) and, for DUP,
    the index of the vector it copies"""

    def __init__(self, kind, lname, n, arr, k, seed=None, dup_of=None):
        self.kind, self.lname, self.n, self.arr, self.k, self.seed, self.dup_of = kind, lname, n, arr, k, seed, dup_of


def radix_edge_scalars(R, W):
    """the scalars on the digit boundaries of radix R (the list of test_radix_r_digits_through_the_tables): R/2, R/2 +- 1, t R^j + e"""
    edge = [0, 1, R // 2 - 1, R // 2, R // 2 + 1, R - 1, R, R + 1, Q - 1, Q - 2, Q // 2, 2 ** 254]
    for j in range(1, W):
        for t in (1, R // 2, R // 2 + 1, R - 1):
            for e in (-1, 0, 1):
                edge.append((t * R ** j + e) % Q)
        edge.append(sum((R // 2) * R ** i for i in range(j + 1)) % Q)
        edge.append(sum((R // 2 - 1) * R ** i for i in range(j + 1)) % Q)
    return edge


def make_vec(kind, lname, m, a, d, seed, edges=None):
    """a vector of `kind` (not DUP) and named length against the 2 m points (a + i d) G.  edges: scalars written over a U vector at
    positions drawn from `seed` (radix widths); the closed form follows them."""
    n, N = length_of(lname, m), 2 * m
    used = min(n, N)                                     # zip() truncation: scalars past the SRS count for nothing
    rnd = random.Random(seed)
    if kind == "U":
        arr = O.splitmix_scalars(n, seed) if n else np.zeros((0, 4), dtype=np.uint64)
        ints = None
        if edges is not None and n >= len(edges):
            arr = arr.copy()
            pos = rnd.sample(range(n), len(edges))
            arr[pos] = _mont(edges)
            seed = None
        if n <= 4096:
            ints = O.fr_array_to_ints(arr)
            k = sum(s * (a + i * d) for i, s in enumerate(ints[:used])) % Q
        else:
            k = O.dot_progression(arr[:used], a, d)      # long vectors: the oracle's C loop (the short ones pin it against Python integers)
        return Vec(kind, lname, n, arr, k, seed)
    if kind == "Z":
        return Vec(kind, lname, n, np.zeros((n, 4), dtype=np.uint64), 0)
    if kind in ("ONE", "TOP", "EQ"):
        val = {"ONE": 1, "TOP": Q - 1}.get(kind) or rnd.randrange(2, Q - 1)
        return Vec(kind, lname, n, np.tile(O.fr_from_int(val), (n, 1)), val * _sum_points(used, a, d) % Q)
    if kind == "HOT":
        arr = np.zeros((n, 4), dtype=np.uint64)
        if n == 0:
            return Vec(kind, lname, n, arr, 0)
        j, val = rnd.randrange(n), rnd.randrange(2, Q - 1)
        arr[j] = O.fr_from_int(val)
        return Vec(kind, lname, n, arr, val * (a + j * d) % Q if j < N else 0)
    if kind == "SMALL":
        vals = [(i * 7919 + seed) % 65536 for i in range(n)]
        arr = np.zeros((n, 4), dtype=np.uint64)
        if n:
            arr[:] = _mont(vals) if n <= 4096 else _small_mont(vals)
        return Vec(kind, lname, n, arr, sum(v * (a + i * d) for i, v in enumerate(vals[:used])) % Q)
    raise ValueError(kind)


_SMALL_TABLE = []


def _small_mont(vals):
    """Montgomery form of many 16-bit values: one conversion per distinct value"""
    if not _SMALL_TABLE:
        _SMALL_TABLE.append(_mont(range(65536)))
    return _SMALL_TABLE[0][np.asarray(vals, dtype=np.int64)]


# (kind, length) per vector; ("DUP", j) copies vector j of the same call.  k = 2, 3, 4, 5, 8, 9: batches of 2, 3, 4, 4+1, 4+4, 4+4+1.
#   k = 2, 3: TOP at j and ONE at j + 1, both on every point of member 0 (the seam between two bucket sets: the last bucket of set j
#             holds the largest top digit, the first bucket of set j + 1 digit 1), all vectors full length on member 0
#   k = 4:    a length-1 vector first, Z and the empty polynomial in the middle, the longest vector last
#   k = 5:    every vector <= m: member 1 gets nothing; a DUP inside one batch
#   k = 8, 9: every kind and every length, TOP / ONE neighbours inside a batch, Z and the empty polynomial in the middle of a batch; k = 9
#             puts a full-length vector and its DUP side by side in one batch (two bucket sets of one sort, on both members)
CALL_SPECS = {
    2: [("TOP", "2m"), ("ONE", "2m")],
    3: [("EQ", "2m"), ("TOP", "2m+9"), ("ONE", "2m-1")],
    4: [("U", "1"), ("Z", "m+1"), ("U", "0"), ("U", "2m+9")],
    5: [("U", "m"), ("SMALL", "m-1"), ("HOT", "m"), ("DUP", 0), ("ONE", "1")],
    8: [("U", "2m"), ("TOP", "m"), ("ONE", "m+1"), ("EQ", "2m-1"), ("SMALL", "m-1"), ("Z", "2m"), ("U", "0"), ("HOT", "2m+9")],
    9: [("U", "2m"), ("DUP", 0), ("TOP", "2m-1"), ("ONE", "2m"), ("SMALL", "m"), ("Z", "2m"), ("U", "0"), ("U", "m+1"), ("U", "2m+9")],
}
KS = tuple(sorted(CALL_SPECS))


def build_call(k, m, a, d, seed, radix=None):
    """the call of k vectors for members of m points.  radix = (R, W): the first U vector long enough takes the radix-R boundary scalars."""
    edges = radix_edge_scalars(*radix) if radix else None
    out = []
    for j, (kind, arg) in enumerate(CALL_SPECS[k]):
        if kind == "DUP":
            src = out[arg]
            out.append(Vec("DUP", src.lname, src.n, src.arr.copy(), src.k, src.seed, dup_of=arg))
            continue
        v = make_vec(kind, arg, m, a, d, seed * 64 + j, edges)
        if edges is not None and kind == "U" and v.seed is None:
            edges = None                                 # placed once per call
        out.append(v)
    return out


def check_call(vecs, m):
    """the conditions every call keeps (asserted on the CPU for every shape's lists)"""
    for v in vecs:
        assert v.kind in KINDS and v.lname in LENGTHS and v.n == length_of(v.lname, m) == len(v.arr)
    live = [(j, v) for j, v in enumerate(vecs) if v.k != 0]
    for x, (j, v) in enumerate(live):
        for i, u in live[:x]:
            assert (u.k != v.k) or v.dup_of == i, ("two vectors with one closed form", i, j)
            assert (u.k == v.k) == (v.dup_of == i)
    for j, v in enumerate(vecs):
        if v.kind == "DUP":
            assert v.dup_of < j and (vecs[v.dup_of].arr == v.arr).all()


def has_top_one_pair(vecs, m):
    """TOP at j and ONE at j + 1 inside one batch, both covering at least member 0's m points"""
    return any(u.kind == "TOP" and v.kind == "ONE" and j % BATCH != BATCH - 1 and u.n >= m and v.n >= m
               for j, (u, v) in enumerate(zip(vecs, vecs[1:])))


def has_zero_and_empty_in_the_middle(vecs):
    """a Z vector and a length-0 polynomial that are neither first nor last in their batch"""
    mid = [v for j, v in enumerate(vecs) if 0 < j % BATCH and j + 1 < min(len(vecs), (j // BATCH + 1) * BATCH)]
    return any(v.kind == "Z" and v.n > 0 for v in mid) and any(v.n == 0 for v in mid)


# (c, m, {J: expected path of member 0 for J full-length vectors}): the shapes of the batched-MSM tests.  Fields not listed per J are
# common to the row.  fixup: 0 per bucket, 1 per edge.
def _row(c, m, js, W, pb, packed, flat, wide8, fixup, n_wide, radix=0):
    pbs = pb if isinstance(pb, dict) else {j: pb for j in js}
    return (c, m, {j: {"J": j, "c": c, "W": W, "radix": radix, "sort": 2, "pb": pbs[j], "packed": packed, "flat": flat, "wide8": wide8,
                       "fixup": fixup, "n_wide": n_wide} for j in js})


RADIX = {21: 0xD0000, 22: 0x288000, 24: 0x9C0000}      # live buckets of the radix-R widths (tests/test_radix_digits.py)
SHAPES = [
    # smallest; m is not a multiple of the 64-scalar slice.  J = 2: 32 * 300 * 2 = 19 200 entries, 9 600 per half < 12 288: one final run
    _row(8, 300, (4, 3, 2), 32, {4: 1, 3: 1, 2: 0}, 1, 0, 0, 0, 0),
    _row(10, 65, (4,), 26, 0, 1, 0, 0, 1, 0),           # one final run (n_final = 1, no long-run kernels); a slice spans two vectors
    _row(13, 5, (4,), 20, 0, 1, 0, 0, 1, 0),            # five scalars per vector
    _row(16, 9000, (2,), 16, 4, 1, 0, 0, 1, 3),         # fused levels 0+1 over a forest of two
    _row(17, 20000, (3,), 16, 6, 1, 0, 0, 1, 5),        # parts > 1; total = 3 * 2^16 is not a power of two
    _row(19, 40000, (3,), 14, 9, 1, 1, 0, 1, 8),        # packed by raising pb; flat write-out
    _row(20, 17, (4,), 13, 6, 1, 0, 0, 1, 9),           # 884 entries into 2^21 buckets (tables whatever the length)
    _row(20, 1, (4,), 13, 6, 1, 0, 0, 1, 9),            # one scalar per vector
    _row(22, 70000, (4,), 12, 12, 1, 1, 0, 1, 12, RADIX[22]),     # radix-R digits with J = 4; pb = PART_MAX_BITS
    _row(24, 130000, (2,), 11, 9, 0, 0, 0, 1, 13, RADIX[24]),     # two-word records, partition-major
    _row(24, 100000, (4,), 11, 10, 0, 1, 0, 1, 14, RADIX[24]),    # two-word records, flat; 2^25 leaves
    _row(21, 270000, (3,), 13, 9, 0, 0, 1, 1, 10, RADIX[21]),     # wide8 with radix-R digits and J = 3
]
DEVICE_GENERATED_FROM = 70000          # the four largest shapes: U vectors are generated in HBM (synthetic_scalars_device)


def shape_seed(c, m):
    return 0xBA7C000 + 4096 * c + m % 4096


def progression(c, m):
    """(a, d) of the shape's SRS: P_i = (a + i d) G"""
    rnd = random.Random(0x5125 + 1000003 * c + m)
    return rnd.randrange(1, Q), rnd.randrange(1, Q)
