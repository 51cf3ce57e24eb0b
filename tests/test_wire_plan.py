"""CPU checks of csrc/wire_plan.hpp: the rules bp_circuit_load_wires sorts and links by (pass count, digit, tile, grids, buffer bytes)
and its host restatement of sort + link, tile by tile and chunk by chunk as the kernels of wire_kernels.hpp take them.  No GPU: the
header is compiled for the host alone (tests/cpp/wire_plan_host.hip).  The reference for S1 S2 S3 is bp_make_s_polynomials, itself
pinned to the reference's unit test by tests/test_circuit_frontend.py; the reference for the cell map is a Python dictionary of lists
(tests/wire_circuits.expected_target)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from tests import general_circuits as G
from tests import wire_circuits as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wp(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("wire_plan") / "libwireplan.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "wire_plan_host.hip"), "-o", so])
    lib = C.CDLL(so)
    lib.wp_consts.restype, lib.wp_consts.argtypes = None, [C.c_void_p]
    lib.wp_passes.restype, lib.wp_passes.argtypes = C.c_uint32, [C.c_uint32]
    lib.wp_digit.restype, lib.wp_digit.argtypes = C.c_uint32, [C.c_uint32, C.c_uint32]
    lib.wp_plan.restype, lib.wp_plan.argtypes = C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p]
    lib.wp_sort_link.restype, lib.wp_sort_link.argtypes = C.c_uint32, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def consts(wp):
    out = (C.c_uint64 * 6)()
    wp.wp_consts(out)
    return dict(zip(("tile", "scan_chunk", "scan_tiles", "block", "radix", "scatter_lds"), out))


def sizes(wp):
    """log_n 3 and 4, and the sizes whose 3n cells lie just below and just above one tile and one scan workgroup's worth of tiles, read
    from the compiled header"""
    k = consts(wp)
    out = [3, 4]
    for edge in (k["tile"], k["tile"] * k["scan_tiles"]):
        below = max(l for l in range(3, 25) if 3 << l < edge)
        assert 3 << below < edge < 3 << (below + 1)
        out += [below, below + 1]
    return sorted(set(out))


def sort_link(wp, ids):
    n = ids.shape[0]
    s = [np.zeros((n, 4), dtype=np.uint64) for _ in range(3)]
    target = np.zeros(3 * n, dtype=np.uint32)
    flat = np.ascontiguousarray(ids, dtype=np.uint32)
    passes = wp.wp_sort_link(n.bit_length() - 1, flat.ctypes.data, s[0].ctypes.data, s[1].ctypes.data, s[2].ctypes.data, target.ctypes.data)
    return s, target, passes


def test_constants_and_pass_rules(wp):
    k = consts(wp)
    assert k["radix"] == 256 and k["block"] == 256 and k["block"] % 64 == 0
    assert k["tile"] % k["block"] == 0 and k["scan_chunk"] == k["scan_tiles"] * k["radix"]
    assert k["scatter_lds"] == (k["tile"] // 64) * k["radix"] * 4 <= 64 * 1024        # one count per (64 keys, digit), static LDS
    for top, passes in ((0, 0), (1, 1), (255, 1), (256, 2), (65535, 2), (65536, 3), ((1 << 24) - 1, 3), (1 << 24, 4), (1 << 31, 4), ((1 << 32) - 1, 4)):
        assert wp.wp_passes(top) == passes, top
    for key in W.EDGE_IDS + (0, 0x12345678):
        assert [wp.wp_digit(key, p) for p in range(4)] == [(key >> (8 * p)) & 255 for p in range(4)]


def test_plan_covers_every_size(wp):
    k = consts(wp)
    names = ("cells", "passes", "tiles", "hist_entries", "scan_chunks", "cell_blocks", "row_blocks", "key_bytes", "hist_bytes", "sums_bytes", "sort_bytes")
    for log_n in range(3, 25):
        for top in (0, 200, 70000, (1 << 32) - 1):
            out = (C.c_uint64 * 11)()
            assert wp.wp_plan(log_n, top, out) == 1, (log_n, top)
            p = dict(zip(names, out))
            cells = 3 << log_n
            assert p["cells"] == cells and p["passes"] == wp.wp_passes(top)
            assert (p["tiles"] - 1) * k["tile"] < cells <= p["tiles"] * k["tile"]
            assert p["hist_entries"] == 256 * p["tiles"]
            assert (p["scan_chunks"] - 1) * k["scan_chunk"] < p["hist_entries"] <= p["scan_chunks"] * k["scan_chunk"]
            assert (p["cell_blocks"] - 1) * k["block"] < cells <= p["cell_blocks"] * k["block"]
            assert (p["row_blocks"] - 1) * k["block"] < 1 << log_n <= p["row_blocks"] * k["block"]
            assert p["key_bytes"] == 4 * cells and p["hist_bytes"] == 4 * p["hist_entries"] and p["sums_bytes"] == 4 * p["scan_chunks"]
            assert p["sort_bytes"] == (4 * p["key_bytes"] + p["hist_bytes"] + p["sums_bytes"] if p["passes"] else 0)
    out = (C.c_uint64 * 11)()
    assert wp.wp_plan(2, 0, out) == 0 and wp.wp_plan(25, 0, out) == 0


def test_sizes_straddle_the_tile_and_the_scan_chunk(wp):
    k = consts(wp)
    s = sizes(wp)
    assert len(s) == 6, s
    tiles = lambda l: -(-(3 << l) // k["tile"])
    assert [tiles(l) for l in s[:3]] == [1, 1, 1] and tiles(s[3]) == 2
    assert tiles(s[4]) < k["scan_tiles"] < tiles(s[5])


def test_host_sort_and_link_equal_make_s_polynomials(wp):
    """every id shape at every size: S1 S2 S3 byte for byte, the pass count, and the cell map a permutation whose cycles are exactly
    the id groups in row-major order"""
    seen = set()
    for log_n in sizes(wp):
        n = 1 << log_n
        for name, (ids, passes) in W.id_shapes(n).items():
            s, target, ran = sort_link(wp, ids)
            assert ran == passes, (log_n, name)
            seen.add(ran)
            want = bp.make_s_polynomials(ids)
            for col in range(3):
                assert s[col].tobytes() == want[col].tobytes(), (log_n, name, col)
            t = target.tolist()
            assert sorted(t) == list(range(3 * n)), (log_n, name)
            assert t == W.expected_target(ids), (log_n, name)
    assert seen == {0, 1, 2, 3, 4}


def test_reference_case_is_among_the_shapes(wp):
    ids, passes = W.id_shapes(8)["reference_case"]
    assert passes == 1 and ids[:2].tolist() == [[1, 2, 3], [1, 4, 2]]
    s, target, _ = sort_link(wp, ids)
    w = bp.scalar_to_int(bp.root_of_unity(8))
    assert bp.scalar_to_int(s[0][0]) == w and bp.scalar_to_int(s[1][0]) == 3 * w % W.Q         # program.rs:229-231


@pytest.mark.parametrize("shape", W.SHAPES + (W.NO_PUBLIC,), ids=["n16", "n128", "n1024", "n128_no_public"])
def test_general_wire_circuit_is_general_circuit_with_numbers(wp, shape):
    """the same gates, witness, publics and sigma as tests/general_circuits.py gives by name; the assignment expands to the columns"""
    c = W.general_wire_circuit(*shape)
    cols, pk, public_column, publics = G.general_circuit(*shape)
    assert c["cols"] == cols and c["public_column"] == public_column and c["publics"] == publics
    assert all(c["sel"][k] == pk[k] for k in W.SELECTORS)
    sig = bp.make_s_polynomials(c["ids"])
    assert [bp.scalars_to_ints(x) for x in sig] == [pk["s1"], pk["s2"], pk["s3"]]
    s, target, _ = sort_link(wp, c["ids"])
    assert all(s[k].tobytes() == sig[k].tobytes() for k in range(3))
    n, ids, values = shape[0], c["ids"], c["values"]
    assert values[0] == 0 and int(ids.max()) == len(values) - 1
    assert [[values[ids[r, j]] for r in range(n)] for j in range(3)] == cols
    assert [(-values[ids[r, 0]]) % W.Q if r < c["n_public"] else 0 for r in range(n)] == public_column
