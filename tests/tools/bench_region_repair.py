"""What the nearest-pathable repair of cell arrival fields costs on the reference, on one core of this machine's CPU:
N_CellArrivalFieldUpdateToNearestPathable through ctypes (tests/region_repair_ref.py) over the requests that
scripts/bench_secondary.py gives the device (`region_repair`): 64 and 256 repairs of dim 96 on a map with blocked blobs.
The answers are compared with the numpy model on the first rows.

    python tests/tools/bench_region_repair.py            # the reference, one JSON line
    python scripts/bench_secondary.py --region-repair-only   # the device, the same requests

`world` is the one place that draws the map and the requests."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DIM, MAP = 96, 4


def world(n, seed=9):
    """A MAP x MAP-chunk map of cost 1 with 400 blocked blobs (3 .. 9 tiles a side, some on cost-255 ground), and n
    repairs: a unit on a blob tile, the field's centre within 20 tiles of it.  Returns a case dict per request (the layout
    of tests/region_repair_cases.py; the worlds share cost and blk)."""
    rng = np.random.RandomState(seed)
    S = MAP * 64
    cost, blk = np.ones((S, S), np.uint8), np.zeros((S, S), np.uint16)
    blobs = []
    for k in range(400):
        r, c, h, w = rng.randint(0, S - 9), rng.randint(0, S - 9), rng.randint(3, 10), rng.randint(3, 10)
        blk[r:r + h, c:c + w] += 1
        if k % 4 == 0:
            cost[r + 1:r + h - 1, c + 1:c + w - 1] = 255
        blobs.append((r, c, h, w))
    cases = []
    while len(cases) < n:
        r, c, h, w = blobs[rng.randint(len(blobs))]
        start = (r + rng.randint(h), c + rng.randint(w))
        centre = tuple(int(v) for v in np.clip(np.array(start) + rng.randint(-20, 21, 2), 0, S - 1))
        case = dict(cost=cost, blk=blk, dim=DIM, centre=centre, start=start, overlay=None, target=centre)
        cases.append(case)
    return cases


def main():
    from tests import region_repair_model as M
    from tests.region_repair_ref import Ref
    out = {}
    for n in (64, 256):
        cases = world(n)
        ok = [c for c in cases if M.status(c["cost"], c["blk"], DIM, c["start"], c["centre"]) == 0]
        noise = np.random.RandomState(1).randint(0, 256, DIM * DIM // 2).astype(np.uint8)
        ref = Ref(ok[0])
        for i, c in enumerate(ok):
            ref.case = c
            got = ref.repair(noise)
            if i < 4:
                assert np.array_equal(got, M.repair(c["cost"], c["blk"], DIM, c["start"], c["centre"], noise)[0])
        out["n%d" % n] = {"repairs": len(ok), "host_rows_left_out": n - len(ok), "ms_one_core": ref.seconds * 1e3,
                          "us_per_repair": ref.seconds * 1e6 / len(ok)}
        ref.close()
    print(json.dumps({"region_repair_reference": out}))


if __name__ == "__main__":
    main()
