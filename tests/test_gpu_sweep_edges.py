"""GPU parity of the sweep's filter and compaction (occ_sweep.hip: k_sw_filter,
k_sw_apply, k_sw_compact, k_sw_ro) on the constructed epochs of
sweep_cases.py, each of which forces one branch at the engine's real
constants: the LDS exact set against the Bloom filter at |C| = 1,024, the
positive-key stash overflowing, tiles past one register round, survivor words
across 64-access boundaries, list lengths around the wave, the workgroup and
the grid, level-1 lists around the serial range, and read-only survivors split
off inside mixed tiles.  test_sweep_cases.py proves on the CPU that every case
has the shape it claims; here the decisions, the commit tn and tnc must be
bit-exact against the oracle's serial replay, and nothing is derived from the
GPU's own output."""
import functools

import numpy as np
import pytest

import _oracle as orc
import deneva_amd as d
import sweep_cases as sc
from deneva_amd._abi import OPT_RO_SPLIT, OPT_SOLVER, OPT_SWEEP_LEVELS

pytestmark = pytest.mark.gpu

SPLIT = [0, 1]
LEVELS = [0, 1, 2]  # auto schedule; one level per host synchronisation; level 1 a serial tail


@pytest.fixture
def sw(engine):
    engine.set_option(OPT_SOLVER, 3)
    yield engine
    engine.set_option(OPT_SOLVER, 0)
    engine.set_option(OPT_SWEEP_LEVELS, 0)
    engine.set_option(OPT_RO_SPLIT, 1)
    engine.tnc = 0


@pytest.fixture(scope="module")
def sharded_engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with d.Engine(devices=[0, 0]) as eng:
        yield eng


@pytest.fixture
def sharded(sharded_engine):
    sharded_engine.set_option(OPT_SOLVER, 3)
    yield sharded_engine
    sharded_engine.set_option(OPT_SOLVER, 0)
    sharded_engine.set_option(OPT_SWEEP_LEVELS, 0)
    sharded_engine.set_option(OPT_RO_SPLIT, 1)
    sharded_engine.tnc = 0


@functools.lru_cache(maxsize=None)
def case(name, *args):
    """(batch, facts, the oracle's (rc, tn, tnc)): built and replayed once."""
    b, facts = getattr(sc, name)(*args)
    return b, facts, orc.occ(b)


def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def run(engine, cs, split, levels=0, batch=None, one_gpu=True):
    b, facts, (erc, etn, etnc) = cs
    engine.set_option(OPT_RO_SPLIT, split)
    engine.set_option(OPT_SWEEP_LEVELS, levels)
    engine.tnc = 0
    rc, tn, st = engine.occ_validate_epoch(b if batch is None else batch, want_tn=True)
    if batch is not None:
        import torch
        torch.cuda.synchronize()
        rc, tn = rc.cpu().numpy(), tn.cpu().numpy()
    rc = np.asarray(rc)
    bad = np.nonzero(rc != erc)[0]
    assert bad.size == 0, f"rc mismatch at {bad[:10]} (gpu {rc[bad[:10]]} oracle {erc[bad[:10]]})"
    assert np.array_equal(np.asarray(tn).astype(np.uint64), etn), "commit tn mismatch"
    assert engine.tnc == etnc
    assert st["n_commit"] == int((erc == 0).sum())
    assert st["n_abort"] == int((erc == 2).sum())
    assert st["peel_prefix"] == sc.P0
    if one_gpu:  # the level-1 list: the survivors the case counts, the read-only ones split off
        assert st["n_survivors"] == facts["surv"] - (facts["ro"] if split else 0)
    return st


@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("c", sc.XCAP_C)
def test_xcap(sw, c, split):
    run(sw, case("xcap_case", c), split)


@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("c", [sc.F_XCAP, sc.F_XCAP + 1])
@pytest.mark.parametrize("variant", sc.STASH_VARIANTS)
def test_stash(sw, variant, c, split):
    run(sw, case("stash_case", variant, 8, c), split)


@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("c", [sc.F_XCAP, sc.F_XCAP + 1])
def test_wide_tile(sw, c, split):
    run(sw, case("wide_tile_case", c), split)


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("L", sc.LIST_SEAMS)
def test_list_seam(sw, L, split, levels):
    run(sw, case("list_seam_case", L), split, levels)


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("extra", [0, 64])
def test_grid_seam(sw, extra, split, levels):
    run(sw, case("grid_seam_case", n_cu(), extra), split, levels)


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("split,s", [(sp, s) for sp in (1, 0) for s in sc.TAIL_S[sp]])
def test_tail_seam(sw, s, split, levels):
    if split and not levels:
        # the auto schedule follows the last epoch's level-1 list: a short one
        # makes level 1 a serial tail of 8,192, a long one restores 3,072
        long_list = s < 4096
        run(sw, case("tail_seam_case", 8193, 1) if long_list else case("list_seam_case", 1), 1, 0)
    st = run(sw, case("tail_seam_case", s, split), split, levels)
    assert st["n_survivors"] == s


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("r", sc.RO_SEAMS)
def test_ro_seam(sw, r, split, levels):
    run(sw, case("ro_seam_case", r), split, levels)


# the key-sharded path: every shard's filter writes kill bits (kill_out), and
# k_sw_apply decides and counts the survivors from their union, survivors with
# no access on a shard included
@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("c", sc.XCAP_C)
def test_sharded_xcap(sharded, c, split):
    run(sharded, case("xcap_case", c), split, one_gpu=False)


@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("variant,per", [(v, 8) for v in sc.STASH_VARIANTS] + [("over", 16)])
def test_sharded_stash(sharded, variant, per, split):
    # per = 16: each of the two shards still sees more than F_STASH positives
    run(sharded, case("stash_case", variant, per, sc.F_XCAP), split, one_gpu=False)


@pytest.mark.parametrize("split", SPLIT)
def test_sharded_wide_tile(sharded, split):
    run(sharded, case("wide_tile_case", sc.F_XCAP), split, one_gpu=False)


@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("L", [63, 64, 65, 257])
def test_sharded_list_seam(sharded, L, split):
    run(sharded, case("list_seam_case", L), split, one_gpu=False)


@pytest.mark.parametrize("split", SPLIT)
def test_device_batch_capture_and_replays(sw, split):
    cs = case("stash_case", "over", 8, sc.F_XCAP)
    db = cs[0].to_torch("cuda:0")
    for _ in range(3):  # the capture, then two replays of the graph
        run(sw, cs, split, batch=db)
