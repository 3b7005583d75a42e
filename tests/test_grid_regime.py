"""CPU: every case of tests/grid_regime.py reaches, at 256 CUs, the launch regime its row claims (the GPU tests of
tests/test_gpu_work_lists.py ask the same again for the device they run on), and regime() agrees with hand-worked figures."""
import pytest

import grid_regime as R

CASES = [(n, D) for table in (R.DENSE_CASES, R.PACKED_CASES) for n, c in table.items() for D in c["Ds"]]


@pytest.mark.parametrize("name,D", CASES)
def test_case_reaches_its_regime_at_256_cus(name, D):
    _, missed = R.case_regime(name, D, 256)
    assert not missed, missed


def test_the_cases_cover_every_regime_between_them():
    """the union of the table: partial last rounds, all three hpw, tail on / off, tickets on / off with both block orders
    and a remainder, extras with and without tickets, row split, side stream on / off, holes, strips"""
    rs = [R.case_regime(n, D, 256)[0] for n, D in CASES]
    assert {r["hpw"] for r in rs} == {1, 2, 4}
    assert any(r["last_round"] < r["G"] for r in rs) and any(r["last_round"] % 8 for r in rs)
    assert {r["dq_tail"] for r in rs} == {True, False} and {r["dq_side_stream"] for r in rs} == {True, False}
    tick = [r for r in rs if r["tickets"]]
    assert any(r["nG_and_7"] == 0 for r in tick) and any(r["nG_and_7"] != 0 and r["n_base_and_7"] != 0 for r in tick)
    assert all(r["n_extra"] > 0 for r in tick) and any(r["row_split"] and not r["tickets"] for r in rs)
    assert any(r["valid_items"] < r["items"] for r in rs) and any(r["dq"].startswith("dqstripasm") for r in rs)


def test_regime_on_hand_worked_shapes():
    # one (batch, KV head) unit of 65536 rows at group 4: four full rounds, too few for the tail
    r = R.regime(1, 4, 1, 65536, 128, 4, 4096, 256)
    assert (r["hpw"], r["items"], r["G"], r["rounds"], r["dq_tail"], r["dq_tail_first"]) == (4, 1024, 256, 4, False, None)
    # one round, no tickets, no tail: what almost every small test shape gets
    r = R.regime(2, 8, 2, 640, 128, 4, 200, 256)
    assert (r["items"], r["G"], r["rounds"], r["last_round"], r["tickets"], r["dq_tail"]) == (40, 40, 1, 40, False, False)
    # more items than 256 lists of 256: the grid grows past the CU count and the tail is off
    r = R.regime(1, 4, 1, 64 * 70000, 128, 4, 300, 256)
    assert r["G"] == 274 and r["rounds"] == 256 and not r["dq_tail"]
    # a device with fewer CUs moves the thresholds
    assert R.regime(7, 7, 7, 2600, 128, 4, 300, 304)["tickets"] is False
    # sink split: block 0 sweeps every row (dkdv_asm_slices), an ordinary block its keys' rows + the window
    assert R.dkdv_asm_slices(0, 2600, 2600, 4, 300) == 82 and R.dkdv_asm_slices(1, 2600, 2600, 4, 300) == 18
    assert R.sink_split_plan(2600, 2600, 4, 300, False, 256)[:2] == (5, 18)
    assert R.sink_split_plan(2600, 2600, 0, 300, False, 256)[0] == 1 and R.sink_split_plan(2600, 2600, 4, 300, True, 256)[0] == 1
