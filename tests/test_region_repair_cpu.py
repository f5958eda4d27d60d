"""tests/region_repair_model.py held against the reference (oracle/_ref): N_CellArrivalFieldUpdateToNearestPathable, exported
by the reference's library, called through ctypes with pfref_nav_private() on every case of tests/region_repair_cases.py
(the NAVHIP_RR_HOST rows excepted: the reference asserts there), on two input fields each.  Every case's premise is asserted
from the model, and each wrong model of region_repair_model.WRONG changes bytes on some case.  No GPU.  The reference's side is
tests/region_repair_ref.py, which tests/test_region_repair_gpu.py uses too."""
import numpy as np
import pytest

from oracle import pfref
from tests import region_repair_cases as rc
from tests import region_repair_model as M
from tests.region_repair_ref import Ref

pytestmark = pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")

NAMES = sorted(rc.CASES)


def model(case, field, **kw):
    return M.repair(case["cost"], case["blk"], case["dim"], case["start"], case["centre"], field, overlay=case["overlay"],
                    target=case["target"], **kw)


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_reference(name):
    """Byte for byte, on the Create field and on random nibbles; the model's Create is the reference's; the premise holds;
    `enemies` plays no part in the reference."""
    case = rc.get(name, M)
    ref = Ref(case)
    assert np.array_equal(case["field"], ref.create())
    assert M.status(case["cost"], case["blk"], case["dim"], case["start"], case["centre"]) == 0
    for key in ("field", "noise"):
        out, info = model(case, case[key])
        got = ref.repair(case[key])
        bad = np.flatnonzero(got != out)
        assert len(bad) == 0, (name, key, len(bad), bad[:8].tolist())
        if key == "field":
            case["premise"](case, out, info, M)
            assert info["written"].any() and not np.array_equal(out, case["field"])
        else:
            # every nibble the repair does not own survives
            keep = ~info["written"]
            assert np.array_equal(M.unpack(out, case["dim"])[keep], M.unpack(case["noise"], case["dim"])[keep])
    assert np.array_equal(ref.repair(case["field"], enemies=0x7fff), model(case, case["field"])[0])
    ref.close()


def test_host_rows_are_what_the_model_says():
    for name, case in rc.host_cases().items():
        assert M.status(case["cost"], case["blk"], case["dim"], case["start"], case["centre"]) == M.RR_HOST, name
    a = rc.get("blob", M)
    assert M.status(a["cost"], a["blk"], a["dim"], a["start"], (128, 70)) == M.RR_HOST             # the centre off the map


@pytest.mark.parametrize("wrong", M.WRONG)
def test_each_wrong_model_changes_bytes(wrong):
    hit = []
    for name in NAMES:
        case = rc.get(name, M)
        if not np.array_equal(model(case, case["field"], wrong=wrong)[0], model(case, case["field"])[0]):
            hit.append(name)
    assert hit, wrong
