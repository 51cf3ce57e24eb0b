"""CPU checks of csrc/ntt_plan.hpp: the LDS tile layout the NTT kernels address and the host sizes, the kernels' limits, and the plan
of a transform under every experiment knob; no GPU: the header is compiled for the host alone (tests/cpp/ntt_plan_host.hip).
Every expectation is written out below -- the default plans as literals, the knob rules as a Python restatement of the driver this
header replaced (make_ntt_plan, pass_threads, swizzled, tile_lds of csrc/ntt.hip), the validity rules from the kernels' index
arithmetic; none comes from the header under test."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO = 0xFFFFFFFF
U32x11, U32x24, U32x7, U32x5 = C.c_uint32 * 11, C.c_uint32 * 24, C.c_uint32 * 7, C.c_uint32 * 5
KIB = 1024


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("ntt_plan") / "libnttplan.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "ntt_plan_host.hip"), "-o", so])
    lib = C.CDLL(so)
    u32, i32, p = C.c_uint32, C.c_int, C.POINTER(C.c_uint32)
    for name, res, args in (("np_default_knobs", None, [p, p, p]), ("np_plan", i32, [u32, p, p, p]), ("np_full_tables", i32, [u32, u32]),
                            ("np_split_ok", i32, [u32, p, u32]), ("np_tile", None, [u32, u32, i32, p]), ("np_tile_swizzled", i32, [u32, u32, i32]),
                            ("np_tile_at", u32, [i32, u32, u32, u32]), ("np_limits", None, [p])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def knobs(tpf=20, cols=(None, None, None, None), split=None, swizzle=1, lanes=0):
    """the eleven words of the shim; split = (k, l1, l2, l3)"""
    return U32x11(tpf, *[AUTO if c is None else c for c in cols], *(split or (0, 0, 0, 0)), swizzle, lanes)


def plan(lib, k, kn):
    """-> (P, h, [(l, s, cl, swizzled, threads, lds, tiles)]); the words that travel to the kernel agree with the passes"""
    out, dev = U32x24(), U32x11()
    valid = lib.np_plan(k, kn, out, dev)
    assert valid == 1, (k, list(kn))                 # what ntt_plan returns always passes its own check
    P = out[1]
    passes = [tuple(out[3 + 7 * i:10 + 7 * i]) for i in range(P)]
    assert out[0] == k and list(dev[:2]) == [k, P] and dev[10] == out[2]
    if P > 1:
        assert list(dev[2:2 + P]) == [q[0] for q in passes] and list(dev[6:6 + P]) == [q[2] for q in passes]
    return P, out[2], passes


# ---- the layout --------------------------------------------------------------------------------------------------------------------
def tw_slots(l):
    return 2 if (1 << l) < 4 else (1 << l) >> 1


def lds_bytes(l, cl, swz):
    """tile rows x (columns + pad) rounded up to even, + stage twiddles, 36 B each, + 16: the padded and the swizzled form"""
    cols = 1 << cl
    pitch = cols if swz or cols == 1 else cols + 1
    return ((((1 << l) * pitch + 1) & ~1) + tw_slots(l)) * 36 + 16


def swizzle_allowed(l, cl):
    return cl == 3 and 2 <= l <= 7


def tile_at(swz, row, c, pitch):
    if not swz:
        return row * pitch + c
    z = (bin(row & 0x54).count("1") & 1) | ((bin(row & 0x28).count("1") & 1) << 1)
    return ((row ^ z) << 3) | c


def test_limits(lib):
    out = U32x7()
    lib.np_limits(out)
    assert list(out) == [512, 160 * KIB, 256, 64 * KIB, 256, 10, 10]


@pytest.mark.parametrize("l", range(0, 11))
def test_layout(lib, l):
    """every cell of a tile lies inside its limb plane, cells are distinct, planes stay 8-byte aligned, and the bytes the host asks for
    are the plane, the twiddle slots behind it and 16"""
    for cl, swz in itertools.product(range(4), (0, 1)):
        assert lib.np_tile_swizzled(l, cl, 1) == swizzle_allowed(l, cl) and lib.np_tile_swizzled(l, cl, 0) == 0
        if swz and not swizzle_allowed(l, cl):
            continue
        t = U32x5()
        lib.np_tile(l, cl, swz, t)
        pitch, tstride, tw_off, slots, nbytes = t
        rows, cols = 1 << l, 1 << cl
        assert pitch == (cols if swz or cols == 1 else cols + 1)
        assert tstride % 2 == 0 and tw_off == 9 * tstride and slots == tw_slots(l)
        assert nbytes == (tstride + slots) * 36 + 16 == lds_bytes(l, cl, swz)
        cells = [lib.np_tile_at(swz, row, c, pitch) for row in range(rows) for c in range(cols)]
        assert cells == [tile_at(swz, row, c, pitch) for row in range(rows) for c in range(cols)]
        assert max(cells) < tstride and len(set(cells)) == rows * cols


def test_old_and_exact_fit_rule_agree():
    """the driver this header replaced tested an override against a conservative size (always padded, + 2 slots); the exact size gives
    the same verdict for every tile shape, so no override changes outcome"""
    for l, cl in itertools.product(range(1, 11), range(4)):
        old = ((1 << l) * ((1 << cl) + 1) + tw_slots(l) + 2) * 36 + 16 > 160 * KIB
        for swz in (False, True) if swizzle_allowed(l, cl) else (False,):
            assert old == (lds_bytes(l, cl, swz) > (64 if swz else 160) * KIB), (l, cl, swz)


# ---- default plans, as literals ------------------------------------------------------------------------------------------------------
SMALL_LDS = [160, 160, 232, 448, 880, 1744, 3472, 6928, 13840, 27664, 55312]
DEFAULT = {      # k: (widths, cl, swizzled, LDS bytes, threads)
    11: ((6, 5), (3, 3), (1, 1), (19600, 9808), (128, 64)),
    12: ((6, 6), (3, 3), (1, 1), (19600, 19600), (128, 128)),
    13: ((7, 6), (3, 3), (1, 1), (39184, 19600), (256, 128)),
    14: ((7, 7), (3, 3), (1, 1), (39184, 39184), (256, 256)),
    15: ((8, 7), (2, 3), (0, 1), (50704, 39184), (256, 256)),
    16: ((8, 8), (2, 2), (0, 0), (50704, 50704), (256, 256)),
    17: ((9, 8), (1, 2), (0, 0), (64528, 50704), (256, 256)),
    18: ((9, 9), (1, 1), (0, 0), (64528, 64528), (256, 256)),
    19: ((10, 9), (1, 1), (0, 0), (129040, 64528), (512, 256)),
    20: ((7, 6, 7), (3, 3, 3), (1, 1, 1), (39184, 19600, 39184), (256, 128, 256)),
    21: ((7, 7, 7), (3, 3, 3), (1, 1, 1), (39184, 39184, 39184), (256, 256, 256)),
    22: ((8, 7, 7), (2, 3, 3), (0, 1, 1), (50704, 39184, 39184), (256, 256, 256)),
    23: ((8, 8, 7), (2, 2, 3), (0, 0, 1), (50704, 50704, 39184), (256, 256, 256)),
    24: ((8, 8, 8), (2, 2, 2), (0, 0, 0), (50704, 50704, 50704), (256, 256, 256)),
    25: ((9, 8, 8), (1, 2, 2), (0, 0, 0), (64528, 50704, 50704), (256, 256, 256)),
    26: ((9, 9, 8), (1, 1, 2), (0, 0, 0), (64528, 64528, 50704), (256, 256, 256)),
    27: ((9, 9, 9), (1, 1, 1), (0, 0, 0), (64528, 64528, 64528), (256, 256, 256)),
    28: ((10, 9, 9), (1, 1, 1), (0, 0, 0), (129040, 64528, 64528), (512, 256, 256)),
}


def test_default_knobs(lib):
    w, full, group = U32x11(), C.c_uint32(), C.c_uint32()
    lib.np_default_knobs(w, C.byref(full), C.byref(group))
    assert list(w) == list(knobs()) and (full.value, group.value) == (24, 22)
    assert [lib.np_full_tables(k, 24) for k in (11, 24, 25, 28)] == [1, 1, 0, 0] and lib.np_full_tables(11, 0) == 0


@pytest.mark.parametrize("k", range(0, 29))
def test_default_plan(lib, k):
    P, h, passes = plan(lib, k, knobs())
    assert h == (k + 1) // 2
    if k <= 10:
        assert P == 1 and passes[0][0] == k and passes[0][3:] == (0, 256, SMALL_LDS[k], 1)
        return
    widths, cl, swz, lds, threads = DEFAULT[k]
    assert P == len(widths) and sum(widths) == k
    for i, q in enumerate(passes):
        last = i + 1 == P
        assert q == (widths[i], 0 if last else sum(widths[i + 1:]), cl[i], swz[i], threads[i], lds[i], 1 << (k - widths[i] - cl[i])), (k, i)


@pytest.mark.parametrize("k", range(0, 29))
def test_group_split(lib, k):
    """2^11 = 2^6 x 2^5 has four column tiles: it does not split over 8 members; every other multi-pass size splits over 2, 4 and 8"""
    for parts in range(0, 18):
        want = k >= 11 and parts in (2, 4, 8) and (k, parts) != (11, 8)
        assert lib.np_split_ok(k, knobs(), parts) == want, (k, parts)


# ---- every knob: the driver's rules restated, then the plan judged as a whole -----------------------------------------------------------
def cols_default(l):
    return 3 if l <= 7 else 2 if l == 8 else 1


def asked_plan(k, tpf=20, cols=(None, None, None, None), split=None, swizzle=1, lanes=0):
    """what the knobs ask for: [(l, s, cl, swizzled, threads, lds, tiles)], as make_ntt_plan / swizzled / pass_threads / tile_lds computed it
    (threads: LANES_SHIFT applies before the clamp to the chosen kernel's bound)"""
    P = 2 if k <= 20 else 3
    if P == 2 and k >= tpf:
        P = 3
    rem, ls, cls = k, [], []
    for i in range(P):
        l = (rem + P - i - 1) // (P - i)
        rem -= l
        cl = cols_default(l)
        over = cols[0 if l <= 7 else l - 7]
        if over is not None:
            cl = over
        if ((1 << l) * ((1 << cl) + 1) + tw_slots(l) + 2) * 36 + 16 > 160 * KIB:
            cl = cols_default(l)
        ls.append(l)
        cls.append(cl)
    if P == 3 and ls[0] <= 7 and ls[0] == ls[1] and ls[2] + 1 == ls[1]:
        ls[1], ls[2] = ls[2], ls[1]
        cls[1:] = [cols_default(l) for l in ls[1:]]
    if split and split[0] == k and sum(split[1:]) == k and max(split[1:]) <= 10 and split[1] >= 2 and split[2] >= 1:
        ls = list(split[1:4] if split[3] else split[1:3])
        cls = [cols_default(l) for l in ls]
    out = []
    for i, (l, cl) in enumerate(zip(ls, cls)):
        swz = int(bool(swizzle) and swizzle_allowed(l, cl))
        threads = min(max(((1 << l) << cl >> 2) << lanes, 64), 256 if swz else 512)
        out.append((l, 0 if i + 1 == len(ls) else k - sum(ls[:i + 1]), cl, swz, threads, lds_bytes(l, cl, swz), (1 << k) >> (l + cl)))
    return out


def valid(k, passes):
    """the validity list: widths sum to k, each <= 10; a strided tile's columns exist (s >= cl), the last pass's rows e_1 exist
    (l_1 >= cl); LDS and threads within the chosen kernel's limits"""
    if sum(q[0] for q in passes) != k or any(q[0] > 10 for q in passes):
        return False
    for i, (l, s, cl, swz, threads, lds, tiles) in enumerate(passes):
        if (passes[0][0] < cl) if i + 1 == len(passes) else (s < cl):
            return False
        if lds > (64 if swz else 160) * KIB or threads > (256 if swz else 512) or tiles < 1:
            return False
    return True


def check(lib, k, **kn):
    P, h, got = plan(lib, k, knobs(**kn))
    assert h == (k + 1) // 2
    if k <= 10:
        assert P == 1 and got[0][0] == k and got[0][4:6] == (256, SMALL_LDS[k])
        return got
    want = asked_plan(k, **kn)
    if not valid(k, want):
        want = asked_plan(k)                         # an override that gives an invalid plan is ignored as a whole
    assert valid(k, want) and got == want, (k, kn, got, want)
    return got


@pytest.mark.parametrize("k", range(0, 29))
def test_every_knob(lib, k):
    some_cols = [(None,) * 4] + [tuple(v if i == j else None for i in range(4)) for j in range(4) for v in range(4)] + [(v,) * 4 for v in range(4)]
    for tpf, cols, swizzle, lanes in itertools.product(range(11, 30), some_cols, (0, 1), (0, 1)):
        check(lib, k, tpf=tpf, cols=cols, swizzle=swizzle, lanes=lanes)
    for tpf, cols, swizzle, lanes in itertools.product((11, 20), itertools.product(range(4), repeat=4), (0, 1), (0, 1)):
        check(lib, k, tpf=tpf, cols=cols, swizzle=swizzle, lanes=lanes)


@pytest.mark.parametrize("k", range(0, 29))
def test_every_split(lib, k):
    """every BP_NTT_SPLIT triple with widths 0..10 for this size (and for another: ignored)"""
    for (a, b, c), swizzle, lanes in itertools.product(itertools.product(range(11), repeat=3), (0, 1), (0, 1)):
        if a + b + c == k or (a, b, c) in ((10, 1, 2), (9, 2, 0), (0, 0, 0)) or (lanes == 0 and swizzle == 1 and a + b + c in (k - 1, k + 1)):
            check(lib, k, split=(k, a, b, c), swizzle=swizzle, lanes=lanes)
            if a + b + c == k:
                check(lib, k, split=(k + 1, a, b, c), swizzle=swizzle, lanes=lanes)


def test_named_cases(lib):
    # BP_NTT_LANES_SHIFT=1: the swizzled kernels are bound to 256 lanes
    assert [q[3:5] for q in check(lib, 14, lanes=1)] == [(1, 256), (1, 256)]
    assert [q[3:5] for q in check(lib, 19, lanes=1)] == [(0, 512), (0, 512)]
    # a strided pass with s = 2 < cl = 3: the default 7, 6
    assert [q[:3] for q in check(lib, 13, split=(13, 10, 1, 2))] == [(7, 6, 3), (6, 0, 3)]
    # overrides that were accepted stay accepted, same widths and cl
    assert [q[:3] for q in check(lib, 11, split=(11, 9, 2, 0))] == [(9, 2, 1), (2, 0, 3)]
    assert [q[:3] for q in check(lib, 12, split=(12, 10, 2, 0))] == [(10, 2, 1), (2, 0, 3)]
    assert [q[:3] for q in check(lib, 13, split=(13, 5, 4, 4))] == [(5, 8, 3), (4, 4, 3), (4, 0, 3)]
    assert [q[:3] for q in check(lib, 20, split=(20, 10, 10, 0))] == [(10, 10, 1), (10, 0, 1)]
    assert [q[:3] for q in check(lib, 20, split=(20, 7, 7, 6))] == [(7, 13, 3), (7, 6, 3), (6, 0, 3)]
    assert [q[:3] for q in check(lib, 11, tpf=11)] == [(4, 7, 3), (3, 4, 3), (4, 0, 3)]
    assert [q[:4] for q in check(lib, 12, swizzle=0)] == [(6, 6, 3, 0), (6, 0, 3, 0)]
    assert [q[:3] for q in check(lib, 12, cols=(0, None, None, None))] == [(6, 6, 0), (6, 0, 0)]
    assert [q[2] for q in check(lib, 24, cols=(None, 3, None, None))] == [3, 3, 3]
    assert [q[2] for q in check(lib, 18, cols=(None, None, 2, None))] == [2, 2]
    assert [q[2] for q in check(lib, 18, cols=(None, None, 3, None))] == [1, 1] and lds_bytes(9, 3, False) == 175120 > 160 * KIB
