"""GPU: the MaaT epoch driver at its seams (maat_cases.py; the facts of every
case are proved on the CPU by test_maat_cases.py).  Every case runs through
test_gpu_maat.run: RC, commit timestamps, the row timestamps after the epoch
and n_commit equal the oracle's, bit for bit, and the number of rounds is the
model's."""
import pytest

import maat_cases as mc
from test_gpu_maat import run

pytestmark = pytest.mark.gpu


def check(engine, name, **kw):
    b, rows, facts = mc.build(name)
    rc, st = run(engine, b, rows=rows, **kw)
    if not mc.takes_prefix(b) and not kw.get("rw_all"):
        assert st["rounds"] == facts["rounds"]
    # at the prefix level too: the prefix's rounds plus the survivors' (none
    # when the filter kills every later txn)
    assert st["rounds"] == mc.expected_rounds(name, bool(kw.get("rw_all")))
    return b, rows, st


@pytest.mark.parametrize("name", list(mc.CASES))
def test_case(engine, name):
    check(engine, name)


@pytest.mark.parametrize("name", mc.DEV_CASES)
def test_case_device_pointers(engine, name):
    check(engine, name, dev=True)


@pytest.mark.parametrize("name", mc.RW_ALL_CASES)
def test_case_read_and_prewrite(engine, name):
    """Every access both reads and prewrites its row (the TPC-C path)."""
    check(engine, name, rw_all=True)


def test_epochs_back_to_back(engine):
    """A long epoch leaves nothing behind in the ring, the look-back tags or
    the buffer sets: a short one, a prefix-level one and the long one again."""
    for name in ("chain-300", "wide_ts-lo32", "prefix_chain-1", "chain-74", "composite-65"):
        check(engine, name)
