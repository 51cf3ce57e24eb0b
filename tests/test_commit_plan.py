"""CPU checks of csrc/commit_plan.hpp: which points and scalars lie on which shard of an SRS, and the route k commitments of one call take
(group batch, queued shards, single-device batch, lanes) with its rounds; no GPU: the header is compiled for the host alone
(tests/cpp/commit_plan_host.hip).  Every expectation is a Python restatement of the lines this header replaced -- shard_range of
capi_ctx.hip, the range cut of srs_shards (capi_srs.hip), the slice lines and the interleaved ifs of commit_many and
commit_many_group_batched (capi_msm.hip), with "the launch answered BP_ERR_TOO_LARGE" read off the restated MSM driver of
tests/test_msm_plan.py -- none comes from the header under test.  One deliberate difference from those lines: on ONE device with
BP_COMMIT_BATCH=1 a batch refused at a later round used to be an error; it now takes the lanes like a batch refused at the first round."""
import ctypes as C
import functools
import os
import random
import subprocess

import pytest

from tests.test_msm_plan import TOO_LARGE, parent_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_BATCH, SHARDED, DEVICE_BATCH, LANES = 0, 1, 2, 3
MAX_BATCH, SLOTS, MAX_LANES = 4, 4, 3
WIDTH = {GROUP_BATCH: MAX_BATCH, SHARDED: SLOTS, DEVICE_BATCH: MAX_BATCH, LANES: MAX_LANES}
UNSET = -1


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("commit_plan") / "libcommitplan.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "commit_plan_host.hip"), "-o", so])
    lib = C.CDLL(so)
    u32, u64, i32 = C.c_uint32, C.c_uint64, C.c_int
    p32, p64, pi = C.POINTER(u32), C.POINTER(u64), C.POINTER(i32)
    for name, res, args in (("cp_plan", i32, [u32, p64, p64, p32, u64, i32, p64, i32, i32, pi, pi, pi, i32]), ("cp_shard_range", None, [u64, u64, u64, p64, p64]),
                            ("cp_shard_cut", None, [u64, u64, u64, u64, u64, p64, p64]), ("cp_shard_slice", u64, [u64, u64, u64, u64]), ("cp_widths", None, [pi])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def shim_plan(lib, shards, n_global, lens, group, knob):
    """-> (route, [(base, cnt), ...]); shards: [(first, n, table_c)]"""
    R, k = len(shards), len(lens)
    route, width, rounds = C.c_int(), C.c_int(), (C.c_int * 64)()
    n_rounds = lib.cp_plan(R, (C.c_uint64 * R)(*[s[0] for s in shards]), (C.c_uint64 * R)(*[s[1] for s in shards]), (C.c_uint32 * R)(*[s[2] for s in shards]),
                           n_global, k, (C.c_uint64 * max(k, 1))(*lens), int(group), knob, route, width, rounds, 32)
    assert n_rounds <= 32 and width.value == WIDTH[route.value]
    return route.value, [(rounds[2 * i], rounds[2 * i + 1]) for i in range(n_rounds)]


# ---- the lines this header replaced, restated -----------------------------------------------------------------------------------------
def parent_shard_range(n, r, R):
    base, extra = n // R, n % R
    lo = r * base + min(r, extra)
    return lo, lo + base + (1 if r < extra else 0)


def parent_cut(first, n, n_global, shard_first, shard_n):
    """srs_shards: n cut to the SRS's length first, then to the shard"""
    end = first if first > n_global else first + min(n, n_global - first)
    return max(first, shard_first), min(end, shard_first + shard_n)


def parent_slice(n_j, n_global, shard_first, shard_n):
    nj = min(n_j, n_global)
    return min(nj - shard_first, shard_n) if nj > shard_first else 0


@functools.lru_cache(None)
def launch_refused(lens, table_c, stride):
    """does msm_launch_many answer BP_ERR_TOO_LARGE for these vectors against tables of this width?"""
    got = parent_plan(len(lens), list(lens), table_c, stride, 0, {})
    return got[0] == "refused" and got[1] == TOO_LARGE


def parent_route(shards, n_global, lens, group, knob):
    """commit_many (k >= 1): the route whose results the caller got, after every retreat"""
    k = len(lens)
    if group and k > 1 and shards[0][2] and knob != 0:
        # commit_many_group_batched: BP_ERR_TOO_LARGE for a shard without tables, and from any launch (the first one returns at once, a later
        # one after the batches before it ran and the launched members were waited for): commit_many then queues the commitments one by one
        refused = not all(c for _, _, c in shards)
        for base in range(0, k, MAX_BATCH):
            for first, n, c in shards:
                ls = tuple(parent_slice(n_j, n_global, first, n) for n_j in lens[base:base + MAX_BATCH])
                if sum(ls) == 0:
                    continue
                refused = refused or launch_refused(ls, c, n)
        if not refused:
            return GROUP_BATCH
    if group or k == 1:
        return SHARDED
    _, e_n, c = shards[0]
    n_max = max(min(n_j, e_n) for n_j in lens)
    if c and 8 * n_max >= 1 << c and knob == 1:
        # a refusal at the first round: the lanes.  At a later round the parent returned the error; the plan takes the lanes there too
        if not any(launch_refused(tuple(min(n_j, e_n) for n_j in lens[base:base + MAX_BATCH]), c, e_n) for base in range(0, k, MAX_BATCH)):
            return DEVICE_BATCH
    return LANES


def check(lib, shards, n_global, lens, group, knob):
    route, rounds = shim_plan(lib, shards, n_global, lens, group, knob)
    key = (shards, n_global, lens, group, knob)
    k = len(lens)
    if k:
        assert route == parent_route(shards, n_global, lens, group, knob), key
    # the rounds cover 0 .. k once, in order, none wider than its route's limit
    at = 0
    for base, cnt in rounds:
        assert base == at and 1 <= cnt <= WIDTH[route], key
        at += cnt
    assert at == k and len(rounds) == -(-k // WIDTH[route]), key
    # the slices of vector j over the shards: ascending, disjoint, together exactly [0, min(n_j, n_global))
    for n_j in lens:
        end = 0
        for first, n, _ in shards:
            s = lib.cp_shard_slice(n_j, n_global, first, n)
            assert s == parent_slice(n_j, n_global, first, n) and (s == 0 or first == end), key
            end += s
        assert end == min(n_j, n_global), key
    return route


N_GLOBAL = [1, 7, 8, 1000, 1001, (1 << 20) + 6]


def test_grid(lib):
    rnd = random.Random(0xC0117)
    seen = {GROUP_BATCH: 0, SHARDED: 0, DEVICE_BATCH: 0, LANES: 0}
    for R in range(1, 9):
        for n_global in N_GLOBAL:
            ranges = [parent_shard_range(n_global, r, R) for r in range(R)]
            seams = [lo for lo, _ in ranges[1:]]
            pick = [0, 1, n_global, n_global + 9] + [max(s - 1, 0) for s in seams] + seams + [s + 1 for s in seams]
            for k in range(10):
                for tables in ("all", "none", "one missing"):
                    for c in (6, 16, 20) if tables != "none" else (0,):
                        for knob in (UNSET, 0, 1):
                            for _ in range(8 if R == 1 else 1):      # one device is an eighth of the grid and has two routes of its own
                                missing = rnd.randrange(R)
                                shards = tuple((lo, hi - lo, 0 if tables == "one missing" and r == missing else c) for r, (lo, hi) in enumerate(ranges))
                                lens = tuple(rnd.choice(pick) for _ in range(k))
                                seen[check(lib, shards, n_global, lens, R > 1, knob)] += 1
    assert min(seen.values()) > 100, seen


def test_shard_ranges_and_cuts(lib):
    lo, hi = C.c_uint64(), C.c_uint64()
    for R in range(1, 9):
        for n in N_GLOBAL + [0, R - 1, R, R + 1]:
            ranges = []
            for r in range(R):
                lib.cp_shard_range(n, r, R, lo, hi)
                assert (lo.value, hi.value) == parent_shard_range(n, r, R), (n, r, R)
                ranges.append((lo.value, hi.value))
            assert ranges[0][0] == 0 and ranges[-1][1] == n and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
            edges = sorted({0, 1, n, n + 1, n + 9} | {a + d for a, _ in ranges for d in (-1, 0, 1) if a + d >= 0})
            for first in edges:
                for cnt in (0, 1, 2, n, n + 9, (1 << 64) - 1 - first):          # the last: srs_shards' default, every point from `first` on
                    covered = 0
                    for a, b in ranges:
                        lib.cp_shard_cut(first, cnt, n, a, b - a, lo, hi)
                        assert (lo.value, hi.value) == parent_cut(first, cnt, n, a, b - a), (first, cnt, n, a, b)
                        covered += max(hi.value - lo.value, 0)
                    assert covered == (0 if first > n else min(cnt, n - first)), (first, cnt, n, R)


def test_widths(lib):
    out = (C.c_int * 4)()
    lib.cp_widths(out)
    assert list(out) == [WIDTH[r] for r in (GROUP_BATCH, SHARDED, DEVICE_BATCH, LANES)]


def test_the_edge_of_one_pipeline(lib):
    """The boundary tests/test_gpu_msm_batch.py::test_the_retreat_to_one_by_one computes in its docstring, plan only: c = 16, J = 4, two
    members of m points each; 2 097 215 points per member fit one pipeline, 2 097 216 do not, three vectors of 2 097 216 do."""
    for m, fits in ((2097215, True), (2097216, False)):
        shards, full, short = ((0, m, 16), (m, m, 16)), (2 * m,) * 4, (1000,) * 4
        assert launch_refused((m,) * 4, 16, m) == (not fits) and not launch_refused((m,) * 3, 16, m)
        assert check(lib, shards, 2 * m, full, True, UNSET) == (GROUP_BATCH if fits else SHARDED)
        assert check(lib, shards, 2 * m, full[:3], True, UNSET) == GROUP_BATCH
        assert check(lib, shards, 2 * m, short, True, UNSET) == GROUP_BATCH
        # the first round fits, the second is refused: one by one from the first commitment on, in two rounds of MSM_SLOTS
        assert shim_plan(lib, shards, 2 * m, short + full, True, UNSET) == ((GROUP_BATCH if fits else SHARDED), [(0, 4), (4, 4)])
        assert check(lib, shards, 2 * m, short + full, True, UNSET) == (GROUP_BATCH if fits else SHARDED)
        assert check(lib, shards, 2 * m, short + full, True, 0) == SHARDED
        # one device, on request: the same edge, at the first round and at a later one (the deliberate difference: lanes, not an error)
        one = ((0, m, 16),)
        assert check(lib, one, m, (m,) * 4, False, 1) == (DEVICE_BATCH if fits else LANES)
        assert shim_plan(lib, one, m, short + (m,) * 4, False, 1) == ((DEVICE_BATCH, [(0, 4), (4, 4)]) if fits else (LANES, [(0, 3), (3, 3), (6, 2)]))
        assert check(lib, one, m, (m,) * 4, False, UNSET) == LANES and check(lib, one, m, (m,), False, 1) == SHARDED
