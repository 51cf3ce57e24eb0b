"""CPU checks of csrc/msm_plan.hpp: the limits of the MSM kernels, the experiment knobs and the plan of one MSM pipeline (window width,
digit radix, sort and record form, slices, launch shapes, the bucket tree, every workspace size); no GPU: the header is compiled for the
host alone (tests/cpp/msm_plan_host.hip).  Every expectation is written out below: the plan as a Python restatement of the driver this
header replaced (make_plan and the decision lines of msm_launch_many of csrc/msm.hip), the path words as the library reported them on an
MI355X before the change (tests/golden/msm_paths.json), the validity rules from the kernels' index arithmetic, the table widths as
literals; none comes from the header under test."""
import ctypes as C
import functools
import json
import os
import subprocess

import pytest

from tests.adversarial import radix_of
from tests.test_radix_digits import windows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSET = 0xFFFFFFFF
KIB = 1024
INVALID_ARG, TOO_LARGE = -1, -10
# name, lo, hi, one value outside the range (it must leave the default), in the order of the shim's words
KNOBS = [("BP_MSM_C", 2, 16, 17), ("BP_MSM_CHUNK", 1, 1024, 1025), ("BP_MSM_RADIX", 0, 1, 2), ("BP_MSM_RADIX_FROM", 8, 30, 7),
         ("BP_MSM_RADIX_BITS", 0, 16, 17), ("BP_MSM_PACKED", 0, 2, 3), ("BP_MSM_SORT", 1, 2, 0), ("BP_MSM_PART_SLICE", 64, 4096, 63),
         ("BP_MSM_PART_WIDE8", 0, 1, 2), ("BP_MSM_COUNT_SLICE", 64, 65536, 63), ("BP_MSM_PART_FLAT", 0, 2, 3), ("BP_MSM_FINAL_THREADS", 256, 1024, 255),
         ("BP_MSM_FIXUP", 0, 2, 3), ("BP_MSM_PLANES_WIDE_MIN", 256, 1 << 30, 255)]
OUT_FIELDS = ("empty valid entries n_chunks kb pb rbits vb sort packed flat wide8 l1_pb l1_rb slice n_slices slice1 n_slices1 count_threads "
              "scatter_threads cap part_lds lv0 lv1 gx2 n_sub shift2 scan_tiles n_final final_grid final_threads long_gx long_gy rhist long_cap ctl_words "
              "ctl_zeroed run_ticket acc_grid by_edges fixup_grid quads per_window n_planes Wr n_wide n_steps tmp_slots0 tmp_slots1").split()
WS_FIELDS = ("ctl counts offsets cursors long_list long_scratch tile_sums sorted bucket_sum partial roots window_sum rkeys0 rvals0 rkeys1 rvals1 "
             "run_off run_cnt run_cur run_long planes_tmp0 planes_tmp1").split()
LEVEL01, LEVEL, STEP = 0, 1, 2
TMP0, TMP1, FINAL = 0, 1, 2
# the limits, as the kernels of msm_kernels.hpp were written against them
MAX_C, MAX_TABLE_C, HIST_LOG, MAX_WINDOWS, MAX_BATCH, SCAN_TILE, RADIX_SLICE, PART_MAX_BITS = 16, 24, 15, 128, 4, 4096, 8192, 12
PART_MAX, FIXUP_LONG, FIXUP_LONG_SLICES, PLANES_STEP_LOG, SLOT = 4096, 16, 8, 6, 176


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("msm_plan") / "libmsmplan.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "msm_plan_host.hip"), "-o", so])
    lib = C.CDLL(so)
    u32, u64, i32 = C.c_uint32, C.c_uint64, C.c_int
    p32, p64 = C.POINTER(u32), C.POINTER(u64)
    for name, res, args in (("mp_plan", i32, [u32, p64, u32, u64, i32, p32, p64, p32, p32, p64, p32, C.c_char_p]), ("mp_default_knobs", None, [p32]),
                            ("mp_windows", u32, [u32]), ("mp_table_radix", None, [u32, p32, p32]), ("mp_auto_width", u32, [u64]),
                            ("mp_width_pays", i32, [u32, u64]), ("mp_limits", None, [p64])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def env_words(env):
    return (C.c_uint32 * 14)(*[env.get(name, UNSET) for name, _, _, _ in KNOBS])


_BUF = ((C.c_uint64 * 64)(), (C.c_uint32 * 33)(), (C.c_uint32 * (8 * 24))(), (C.c_uint64 * 22)(), (C.c_uint32 * 12)(), C.create_string_buffer(64))


def shim_plan(lib, J, n_each, table_c, stride, blob, env):
    """-> ("refused", code, text) | ("empty",) | ("plan", out dict, dev words, steps, ws dict, path words)"""
    out, dev, steps, ws, path, what = _BUF
    err = lib.mp_plan(J, (C.c_uint64 * 8)(*(list(n_each) + [0] * 8)[:8]), table_c, stride, blob, env_words(env), out, dev, steps, ws, path, what)
    if err:
        return ("refused", err, what.value.decode())
    if out[0]:
        return ("empty",)
    o = dict(zip(OUT_FIELDS, out))
    return ("plan", o, list(dev), [tuple(steps[8 * i:8 * i + 8]) for i in range(o["n_steps"])], dict(zip(WS_FIELDS, ws)), list(path))


# ---- the driver this header replaced, restated --------------------------------------------------------------------------------------
@functools.lru_cache(None)
def width_of(c):
    """W and the bias words of power-of-two windows, and the radix msm_radix_compute picks for (c, W): (W, bias, (R, m, radix bias))"""
    W = windows_of(c)
    bias = sum(1 << (c * w + c - 1) for w in range(W - 1))
    return W, bias, radix_of(c, W) if c >= 8 else (0, 0, 0)


def words(x, k):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(k)]


def part_slice(slice_, limit, wgs, scalars, staged):
    while slice_ < limit and 2 * slice_ * staged <= 65536 and slice_ * wgs < scalars:
        slice_ <<= 1
    return slice_


def cdiv(a, b):
    return (a + b - 1) // b


def parent_plan(J, n_each, table_c, stride, blob, env):
    def knob(name, dflt, lo, hi):
        v = env.get(name)
        return dflt if v is None or not lo <= v <= hi else v

    if J < 1 or J > MAX_BATCH or (J > 1 and (not table_c or blob)):
        return ("refused", INVALID_ARG, "MSM batch")
    n = max(n_each[:J])
    if n == 0:
        return ("empty",)
    if n >= 1 << 31:
        return ("refused", TOO_LARGE, "MSM length >= 2^31")
    # make_plan
    c = 4 if n < 32 else n.bit_length() - 1 - 3
    c = min(max(c, 4), MAX_C)
    c = knob("BP_MSM_C", c, 2, MAX_C)
    if table_c:
        c = table_c
    c = max(c, 2)
    W, bias, (R, m, rbias) = width_of(c)
    use_radix = bool(table_c) and knob("BP_MSM_RADIX", 1, 0, 1) != 0 and c >= knob("BP_MSM_RADIX_FROM", 21, 8, 30) and R != 0
    B = 1 << (c - 1)
    total = J * B if table_c else W * B
    entries = W * n * J
    chunk_cap = 1024 if table_c else 64
    if table_c and entries <= 1 << 20:
        chunk = entries >> 16
    elif table_c and entries <= 20000000:
        chunk = cdiv(entries, 131072)
    else:
        chunk = cdiv(entries, 262144)
    chunk = min(max(chunk, 4), chunk_cap)
    chunk = knob("BP_MSM_CHUNK", chunk, 1, 1024)
    lanes = 0 if knob("BP_MSM_CHUNK", 0, 1, 1024) else cdiv(entries, chunk)
    dev = ([n, c, W, B, chunk, lanes & 0xFFFFFFFF] + words(rbias if use_radix else bias, 9) +
           [total, 0 if table_c else B, stride & 0xFFFFFFFF if table_c else 0, 1 if B <= 1 << HIST_LOG else B >> HIST_LOG, J] +
           [n_each[j] if j < J else 0 for j in range(4)] + [R if use_radix else 0] + words(m if use_radix else 0, 8))
    # msm_launch_many
    if entries >= 1 << 32:
        return ("refused", TOO_LARGE, "MSM length * windows >= 2^32")
    Wr = J if table_c else W
    n_chunks = cdiv(entries, chunk)
    quads = 1 if table_c else (c + 2) // 4
    per_window = c if table_c else quads
    long_cap = n_chunks // FIXUP_LONG + 1
    ctl_fixed = 8 + PART_MAX + long_cap
    ws = dict.fromkeys(WS_FIELDS, 0)
    ws.update(ctl=(ctl_fixed + 65536) * 4, counts=total * 4, offsets=(total + 1) * 4, cursors=total * 4, long_list=long_cap * 4,
              long_scratch=long_cap * FIXUP_LONG_SLICES * SLOT, tile_sums=4096 * 4, sorted=entries * 4, bucket_sum=total * SLOT, partial=2 * n_chunks * SLOT)
    n_planes = Wr * per_window
    if n_planes > MAX_WINDOWS:
        return ("refused", TOO_LARGE, "MSM windows")
    if not table_c:
        ws["roots"] = W * c * SLOT
    ws["window_sum"] = n_planes * SLOT + 16
    kb = 0
    while (1 << kb) < total:
        kb += 1
    pb = 0
    run_min = 12288 if table_c else 6144
    while pb < kb and (entries >> (pb + 1)) >= run_min:
        pb += 1
    pb = knob("BP_MSM_RADIX_BITS", pb, 0, 16)
    if pb + HIST_LOG < kb:
        pb = kb - HIST_LOG
    pb = min(pb, kb, 16)
    if pb > PART_MAX_BITS and (entries >> PART_MAX_BITS) <= 32768:
        pb = PART_MAX_BITS
    if pb + HIST_LOG < kb:
        pb = kb - HIST_LOG
    wpoints = dev[17]
    idx_max = (n - 1) + (W - 1) * wpoints
    vb = 1
    while (idx_max >> (vb - 1)) != 0:
        vb += 1
    packed_env = knob("BP_MSM_PACKED", 1, 0, 2)
    if packed_env == 1 and kb + vb > 32 + pb and kb + vb - 32 <= PART_MAX_BITS and knob("BP_MSM_RADIX_BITS", 99, 0, 16) == 99:
        pb = kb + vb - 32
    sort = 1 if ((knob("BP_MSM_SORT", 2, 1, 2) == 1 and J == 1 and pb > 0) or pb > PART_MAX_BITS) else 2
    if sort != 2 and J > 1:
        return ("refused", TOO_LARGE, "MSM batch too long for the partition sort")
    rbits, n_final = kb - pb, 1 << pb
    o = dict.fromkeys(OUT_FIELDS, 0)
    o.update(entries=entries, n_chunks=n_chunks, kb=kb, pb=pb, rbits=rbits, vb=vb, sort=sort, n_final=n_final, rhist=(1 << rbits) * 4, long_cap=long_cap,
             ctl_words=ctl_fixed + 65536, ctl_zeroed=ctl_fixed + n_final, run_ticket=ctl_fixed, quads=quads, per_window=per_window, n_planes=n_planes, Wr=Wr)
    packed = flat = wide8 = 0
    ws.update(rkeys0=entries * 4, run_off=(3 * n_final + 16) * 4, run_cur=n_final * 4, run_long=(n_final + 2) * 4)
    if sort == 2:
        packed = int(rbits + vb <= 32 and packed_env != 0)
        rec = 4 if packed else 8
        slice_ = part_slice(64, 1024, 512, n * J, W * rec)
        slice_ = knob("BP_MSM_PART_SLICE", slice_, 64, 4096)
        if slice_ < 64 or slice_ > 4096 or slice_ * W * rec > 65536:
            slice_ = 64
        wide8 = int(not packed and slice_ == 512 and 1024 * 512 < n * J and 3 * n_final * 4 + 1024 * W * 8 <= 156 * KIB and
                    knob("BP_MSM_PART_WIDE8", 1, 0, 1) != 0)
        if wide8:
            slice_ = 1024
        cap, n_slices = slice_ * W, cdiv(n * J, slice_)
        threads = 1024 if slice_ >= 1024 else (256 if slice_ <= 256 else slice_)
        if not packed:
            ws["rvals0"] = entries * 4
        slice1 = part_slice(slice_, 8192, 256, n * J, 0)
        slice1 = knob("BP_MSM_COUNT_SLICE", slice1, 64, 65536)
        n_slices1 = cdiv(n * J, slice1)
        count_threads = 1024 if slice1 >= 1024 else threads
        flat_env = knob("BP_MSM_PART_FLAT", 2, 0, 2)
        flat = 0 if wide8 else int((cap >> pb) < 8 if flat_env == 2 else flat_env == 1)
        part_lds = 3 * n_final * 4 + cap * rec + (cap * 2 if flat else 0)
        final_threads = knob("BP_MSM_FINAL_THREADS", 512 if (entries >> pb) <= 8192 else 1024, 256, 1024) & ~63
        o.update(l1_pb=pb, l1_rb=rbits, final_grid=min(n_final, 4096), final_threads=final_threads)
        if n_final > 1:
            o.update(long_gx=64, long_gy=min(n_final, 4))
    else:
        lv = (pb if pb <= 8 else pb - pb // 2, 0 if pb <= 8 else pb // 2)
        ws.update(rvals0=entries * 4, rkeys1=entries * 4, rvals1=entries * 4, run_cnt=n_final * 4)
        pb1, rb1 = lv[0], kb - lv[0]
        slice_ = part_slice(64, 1024, 512, n, W * 8)
        slice1 = part_slice(slice_, 8192, 256, n, 0)
        cap, n_slices = slice_ * W, cdiv(n, slice_)
        threads = 1024 if slice_ >= 1024 else (256 if slice_ <= 256 else slice_)
        n_slices1 = cdiv(n, slice1)
        count_threads = 1024 if slice1 >= 1024 else threads
        part_lds = 3 * (1 << pb1) * 4 + cap * 8
        runs = 1 << pb1
        o.update(l1_pb=pb1, l1_rb=rb1, lv0=lv[0], lv1=lv[1])
        if lv[1]:
            n_sub = runs << lv[1]
            o.update(n_sub=n_sub, shift2=rb1 - lv[1], gx2=min(cdiv(entries // runs, RADIX_SLICE) + (1 if runs > 1 else 0), 4096), scan_tiles=cdiv(n_sub, SCAN_TILE))
            runs = n_sub
        assert runs == n_final
        o.update(final_grid=min(runs, 4096), final_threads=1024)
        if runs > 1:
            o.update(long_gx=256, long_gy=min(runs, 16))
    o.update(packed=packed, flat=flat, wide8=wide8, slice=slice_, n_slices=n_slices, slice1=slice1, n_slices1=n_slices1, count_threads=count_threads,
             scatter_threads=threads, cap=cap, part_lds=part_lds, acc_grid=cdiv(n_chunks, 256))
    fixup_env = knob("BP_MSM_FIXUP", 0, 0, 2)
    by_edges = int(fixup_env == 2 if fixup_env else entries // total < 2 * chunk)
    o.update(by_edges=by_edges, fixup_grid=cdiv(n_chunks, 256) if by_edges else cdiv(total * (2 if table_c else 1), 256))
    # the tree: the sizing loop, then the launch loop
    levels = c - 1
    wide_min = knob("BP_MSM_PLANES_WIDE_MIN", 24000, 256, 1 << 30)
    n_wide = 0
    while n_wide < levels and (total >> (n_wide + 1)) * (n_wide + 1) >= wide_min:
        n_wide += 1
    if n_wide == levels:
        n_wide = levels - 1
    if n_wide < 2:
        n_wide = 0
    need, kk, flip = [0, 0], 0, 0
    while kk < levels:
        kk += 1 if kk < n_wide else min(levels - kk, PLANES_STEP_LOG)
        if kk < levels:
            need[flip] = max(need[flip], (total >> kk) * (kk + 1))
        flip ^= 1
    steps, k, nodes, flip = [], 0, total, 0
    while k < levels:
        if k == 0 and n_wide:
            nodes >>= 2
            flip ^= 1
            steps.append((LEVEL01, flip, 0, 2, nodes, cdiv(nodes, 256), 1, 0))
            k = 2
        elif k < n_wide:
            nodes >>= 1
            steps.append((LEVEL, flip, k, 1, nodes, cdiv(nodes * (k + 1), 256), 1, 0))
            k += 1
        else:
            m = min(levels - k, PLANES_STEP_LOG)
            nodes >>= m
            steps.append((STEP, FINAL if k + m == levels else flip, k, m, nodes, nodes, k + 1, (2 << m) * SLOT))
            k += m
        flip ^= 1
    o.update(n_wide=n_wide, n_steps=len(steps), tmp_slots0=need[0], tmp_slots1=need[1])
    ws.update(planes_tmp0=need[0] * SLOT, planes_tmp1=need[1] * SLOT)
    path = [J, c, W, R if use_radix else 0, sort, pb, packed, flat, wide8, by_edges, n_wide, chunk]
    return ("plan", o, dev, steps, ws, path)


def valid(o, dev, steps, ws):
    """what the kernels' index arithmetic needs, from the kernels' side"""
    n, c, W, chunk, lanes, total, J = dev[0], dev[1], dev[2], dev[4], dev[5], dev[15], dev[19]
    ok = o["part_lds"] <= 156 * KIB and o["rhist"] <= 144 * KIB and RADIX_SLICE * 9 <= 96 * KIB        # the limits msm_init_device sets
    ok &= all(t % 64 == 0 and 0 < t <= 1024 for t in (o["count_threads"], o["scatter_threads"], o["final_threads"]))
    ok &= o["rbits"] <= HIST_LOG and 1 << o["pb"] <= 65536 and o["pb"] + o["rbits"] == o["kb"] and 1 << o["kb"] >= total
    ok &= o["l1_pb"] <= PART_MAX_BITS and o["n_final"] == 1 << o["pb"]
    ok &= not o["packed"] or o["rbits"] + o["vb"] <= 32
    ok &= o["slice"] * o["n_slices"] >= n * J and o["slice1"] * o["n_slices1"] >= n * J and o["cap"] == o["slice"] * W
    ok &= o["n_chunks"] * chunk >= o["entries"] and (lanes == 0 or lanes * chunk >= o["entries"]) and o["acc_grid"] * 256 >= o["n_chunks"]
    ok &= ws["partial"] >= 2 * o["n_chunks"] * SLOT and ws["long_list"] >= 4 * (o["n_chunks"] // FIXUP_LONG + 1)
    k, covered = 0, []
    for kind, out, k0, m, nodes, gx, gy, lds in steps:                       # levels 0 .. c - 2 exactly once
        covered += list(range(k0, k0 + m))
        k = k0 + m
        ok &= nodes == total >> k and lds <= 64 * KIB and (out == FINAL) == (k == c - 1)
        ok &= out == FINAL or nodes * (k + 1) * SLOT <= ws["planes_tmp%d" % out]
        ok &= gx * gy * (256 if kind != STEP else 1) >= (nodes * (k0 + 1) if kind != LEVEL01 else nodes)
    ok &= covered == list(range(c - 1))
    ok &= o["n_planes"] <= MAX_WINDOWS
    ok &= o["ctl_zeroed"] * 4 <= ws["ctl"] and o["run_ticket"] + o["n_final"] <= o["ctl_zeroed"] and o["run_ticket"] >= 8 + PART_MAX + o["long_cap"]
    return bool(ok)


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 31, 32, 33, (1 << 20) + 6, (1 << 31) - 1] + [(1 << k) + d for k in range(5, 25) for d in (-1, 0, 1)]
WIDTHS = [0] + list(range(4, 25))


def unequal(n, J):
    """J lengths, the longest n"""
    return [n - n // 3, n, max(n // 2, 1), 1][:J] if J > 1 else [n]


def compare(lib, J, n_each, table_c, stride, blob, env):
    got, want = shim_plan(lib, J, n_each, table_c, stride, blob, env), parent_plan(J, n_each, table_c, stride, blob, env)
    key = (J, n_each, table_c, stride, blob, env)
    assert got[0] == want[0], key
    if got[0] != "plan":
        assert got == want, key                                         # a refusal: the parent's code and text
        return got
    _, o, dev, steps, ws, path = got
    assert o.pop("valid") == 1, key                                     # msm_plan_valid holds for every plan returned
    want[1].pop("valid")
    assert valid(o, dev, steps, ws), key
    for name in OUT_FIELDS:
        if name != "valid":
            assert o[name] == want[1][name], (name, key)
    assert dev == want[2], key
    assert steps == want[3] and ws == want[4] and path == want[5], key
    return got


def sweep(lib, env):
    kinds = {"plan": 0, "refused": 0, "empty": 0}
    for n in SIZES:
        for table_c in WIDTHS:
            for J in (1, 2, 3, 4):
                kinds[compare(lib, J, unequal(n, J), table_c, n, 0, env)[0]] += 1
    return kinds


def test_default_knobs_sweep(lib):
    kinds = sweep(lib, {})
    assert kinds["plan"] > 3000 and kinds["refused"] > 200
    for n in (1, 1 << 16, 1 << 20):                                     # a record in HBM: one vector only
        assert compare(lib, 1, [n], 20, n, 1, {})[0] == "plan" and compare(lib, 1, [n], 0, 0, 1, {})[0] == "plan"
        assert compare(lib, 2, [n, n], 20, n, 1, {}) == ("refused", INVALID_ARG, "MSM batch")


@pytest.mark.parametrize("name,lo,hi,bad", KNOBS, ids=[k[0] for k in KNOBS])
def test_each_knob_alone(lib, name, lo, hi, bad):
    """both ends of the range, and a value outside it that leaves the default"""
    for v in (lo, hi):
        sweep(lib, {name: v})
    for n in SIZES:
        for table_c in (0, 16, 20, 22):
            J = 1 if table_c == 0 else 3
            assert shim_plan(lib, J, unequal(n, J), table_c, n, 0, {name: bad}) == shim_plan(lib, J, unequal(n, J), table_c, n, 0, {})
    sweep(lib, {name: bad})


def test_refusals_and_edges(lib):
    assert compare(lib, 1, [0], 0, 0, 0, {}) == ("empty",) and compare(lib, 3, [0, 0, 0], 16, 5, 0, {}) == ("empty",)
    for J in (0, 5, 1 << 31):
        assert shim_plan(lib, J, [5] * 8, 16, 5, 0, {}) == ("refused", INVALID_ARG, "MSM batch")
    assert compare(lib, 2, [5, 5], 0, 0, 0, {}) == ("refused", INVALID_ARG, "MSM batch")
    assert compare(lib, 1, [1 << 31], 0, 0, 0, {}) == ("refused", TOO_LARGE, "MSM length >= 2^31")
    assert compare(lib, 1, [(1 << 31) - 1], 0, 0, 0, {}) == ("refused", TOO_LARGE, "MSM length * windows >= 2^32")
    assert compare(lib, 1, [1 << 28], 20, 1 << 28, 0, {})[0] == "plan"          # 13 * 2^28 < 2^32
    assert compare(lib, 1, [1 << 28], 16, 1 << 28, 0, {}) == ("refused", TOO_LARGE, "MSM length * windows >= 2^32")
    # the literal of tests/test_gpu_msm_batch.py: c = 16, J = 4 is refused from 2 097 216 points per vector on
    assert compare(lib, 4, [2097215] * 4, 16, 2097216, 0, {})[0] == "plan"
    assert compare(lib, 4, [2097216] * 4, 16, 2097216, 0, {}) == ("refused", TOO_LARGE, "MSM batch too long for the partition sort")
    # 128 two-bit windows are the most any width hands to the host: "MSM windows" (more than 128 slots) guards the pinned slot, no input reaches it
    assert compare(lib, 1, [100], 0, 0, 0, {"BP_MSM_C": 2})[1]["n_planes"] == 128
    # a width no table has (bp_srs_precompute builds 4..24): the driver this header replaced indexed past its radix cache here
    assert shim_plan(lib, 1, [100], 25, 100, 0, {}) == ("refused", INVALID_ARG, "MSM table width")


def test_recorded_paths(lib):
    """msm_plan_path reproduces what bp_msm_last_path reported, shipped and experiment builds"""
    records = json.load(open(os.path.join(ROOT, "tests", "golden", "msm_paths.json")))["records"]
    assert len(records) >= 20
    for r in records:
        got = shim_plan(lib, r["J"], r["n_each"], r["table_c"], r["table_stride"], r["blob"], r["env"])
        assert got[0] == "plan" and got[5] == r["path"], r
    assert any(r["path"][:11] == [4, 16, 16, 0, 2, 11, 1, 1, 0, 1, 4] for r in records)      # tests/test_gpu_msm_batch.py's literal
    assert {r["path"][4] for r in records} == {1, 2} and {r["build"] for r in records} == {"shipped", "exp"}


# ---- limits, windows, table widths ------------------------------------------------------------------------------------------------------
def test_limits_and_default_knobs(lib):
    out, w = (C.c_uint64 * 18)(), (C.c_uint32 * 14)()
    lib.mp_limits(out)
    assert list(out) == [16, 24, 15, 128, 4, 4096, 8192, 12, 4096, 16, 8, 2048, 6, 176, 96 * KIB, 144 * KIB, 156 * KIB, 64 * KIB]
    lib.mp_default_knobs(w)
    assert list(w) == [0, 0, 1, 21, 99, 1, 2, 0, 1, 0, 2, 0, 0, 24000]


def test_windows_and_radix(lib):
    for c in range(2, 25):
        assert lib.mp_windows(c) == windows_of(c), c
        for env in ({}, {"BP_MSM_RADIX": 0}, {"BP_MSM_RADIX_FROM": 8}, {"BP_MSM_RADIX_FROM": 30}):
            out = (C.c_uint32 * 18)()
            lib.mp_table_radix(c, env_words(env), out)
            R, m, bias = radix_of(c, windows_of(c)) if c >= 8 else (0, 0, 0)
            if env.get("BP_MSM_RADIX", 1) == 0 or c < env.get("BP_MSM_RADIX_FROM", 21) or R == 0:
                assert list(out) == [0] * 18, (c, env)
            else:
                assert list(out) == [R] + words(m, 8) + words(bias, 9), (c, env)
    assert [lib.mp_windows(c) for c in (4, 16, 20, 22)] == [64, 16, 13, 12]


def test_table_widths(lib):
    """the automatic width of bp_srs_precompute and the rule that says whether tables of a width pay, at every boundary"""
    auto = {1: 4, 1 << 8: 4, (1 << 9) - 1: 4, 1 << 9: 5, 1 << 10: 6, 1 << 12: 8, (1 << 14) - 1: 9, 1 << 14: 16, 1 << 16: 16, (1 << 20) - 1: 16, 1 << 20: 20,
            (1 << 24) - 1: 20, 1 << 24: 22, 1 << 26: 22}
    for n, c in auto.items():
        assert lib.mp_auto_width(n) == c, n
    pays = {(4, 1): 0, (4, 2): 1, (16, (1 << 13) - 1): 0, (16, 1 << 13): 1, (20, 1 << 17): 1, (20, (1 << 17) - 1): 0, (22, 1 << 19): 1, (22, (1 << 19) - 1): 0,
            (24, 1 << 21): 1, (24, (1 << 21) - 1): 0, (22, 1 << 18): 0, (24, 1 << 18): 0}
    # the automatic width always pays for a full-length MSM
    pays.update({(4, 1 << 8): 1, (9, (1 << 14) - 1): 1, (16, 1 << 14): 1, (16, (1 << 20) - 1): 1, (20, 1 << 20): 1, (20, (1 << 24) - 1): 1, (22, 1 << 24): 1})
    for (c, n), want in pays.items():
        assert lib.mp_width_pays(c, n) == want, (c, n)
