"""Every arithmetic primitive of the headers run ON THE CARD, one case per lane, on the adversarial tables of tests/adversarial.py, and
compared with Python integers limb for limb (tests/devcheck/libdevcheck.so: the product's headers built with the product's flags for
gfx950 -- the inline-assembly multiply-accumulate, the Fermat inversions and what hipcc makes of the 28- and 29-bit columns at -O3).
No case is skipped or filtered; a mismatch names the entry point, the case index and the operands in hex, which replay through
libdevcheck_host.so (tests/test_devcheck_host.py).  A missing library is built; if that fails the test FAILS -- it never skips."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import adversarial as A

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "devcheck")
STATE = {"dead": None, "compared": 0}


@pytest.fixture(scope="module")
def dev():
    so = os.path.join(DIR, "libdevcheck.so")
    if not os.path.exists(so):
        try:
            subprocess.check_call(["make", "-C", DIR, "-s", "libdevcheck.so"])
        except Exception as e:                                   # noqa: BLE001 -- any failure to build is a failure of the test
            pytest.fail("tests/devcheck/libdevcheck.so is missing and could not be built with hipcc: %r" % (e,))
    return C.CDLL(so)


@pytest.fixture(scope="module")
def tables(dev):
    b = np.zeros(2 * len(A.BOUND_NAMES), dtype=np.uint64)
    dev.devcheck_bounds.restype = None
    dev.devcheck_bounds(C.c_void_p(b.ctypes.data))
    return A.tables(b)


@pytest.mark.parametrize("name", sorted(A.ENTRY))
def test_device_equals_python_integers(dev, tables, name):
    if STATE["dead"]:
        pytest.fail("not launched: %s" % STATE["dead"])          # after a failed launch nothing more is started on the card
    t = tables[name]
    try:
        compared, bad = A.run_table(dev, t)
    except RuntimeError as e:
        STATE["dead"] = str(e)
        raise
    STATE["compared"] += compared
    print("dc_%s: %d of %d cases compared on the device, %d differ" % (name, compared, len(t.rows), len(bad)))
    assert compared == len(t.rows)
    assert not bad, "%d of %d cases differ\n%s" % (len(bad), compared, "\n".join(bad[:5]))


def test_every_case_was_compared(tables):
    total = sum(len(t.rows) for t in tables.values())
    print("device check: %d of %d cases compared over %d entry points" % (STATE["compared"], total, len(tables)))
    assert STATE["dead"] is None and STATE["compared"] == total
