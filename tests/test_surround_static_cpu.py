"""The numpy model of the static surround arm (tests/surround_static_model.py) is pinned to the reference build: first the
ctypes calling convention it uses for the reference's own functions, then -- on every scene of the GPU file the model can
afford -- N_ObjAdjacentToStaticWith's and N_ClosestReachableAdjacentPosStatic's answers (floats compared as uint32).  A pick
keyed on the answer tile's position, the mistake the tie case is there for, changes an answer.  No GPU; skipped where
oracle/_ref is absent."""
import numpy as np
import pytest

from oracle import pfref
from tests import surround_model as sm
from tests import surround_static_model as ssm

pytestmark = pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")

SCENES = [("axis_aligned",), ("rotated",), ("chunk_corner_and_edge",), ("two_islands",), ("nothing_reachable",), ("window", 154),
          ("window", 155), ("mixed", 257)]


def test_by_value_structures_reach_the_reference_as_its_own_wrapper_passes_them():
    """N_DestIDForPos(void*, vec3_t, vec2_t, enum) called the way the static queries are called equals RefNav.dest_id."""
    w = sm.world("chunk_corner")
    nav = sm.ref_nav(w)
    try:
        ref = ssm.Ref(nav)
        assert [float(v) for v in nav.map_pos] == [ref.mp.x, ref.mp.y, ref.mp.z] == [256.0, 0.0, -256.0]
        got = ssm.map_vec3(2, 2)
        assert (got.x, got.y, got.z) == (ref.mp.x, ref.mp.y, ref.mp.z)
        seen = set()
        for (r, c), layer in (((0, 0), 0), ((63, 64), 0), ((64, 63), 1), ((127, 127), 0), ((5, 100), 3), ((90, 17), 0)):
            p = sm.xz(2, 2, r, c, (0.7, -1.1))
            assert ref.dest_id(p, layer) == nav.dest_id(p, layer)
            seen.add(ref.dest_id(p, layer))
        assert len(seen) == 6
    finally:
        nav.close()


@pytest.mark.parametrize("name", SCENES, ids=lambda s: "_".join(map(str, s)))
def test_model_equals_the_reference(name):
    sc = ssm.scene(*name)
    w = sc.world
    q, d, info = ssm.answers(sc)
    nav = sm.ref_nav(w)
    try:
        for l in w.blockers:
            assert np.array_equal(sm.to_chunks(w.islands), nav.plane(pfref.PLANE_ISLANDS, l))
        rq, rd = ssm.Ref(nav).answers(sc)
    finally:
        nav.close()
    rows = sc.static_rows()
    assert len(rows) > 0
    host = q == sm.SQ_HOST
    assert host.sum() == (len(rows) if name == ("window", 155) else 0)
    assert np.array_equal(q[~host], rq[~host]) and np.array_equal(d[~host].view(np.uint32), rd[~host].view(np.uint32))


def test_a_pick_keyed_on_the_tile_changes_an_answer():
    sc = ssm.scene("rotated")
    q, d, _ = ssm.answers(sc)
    vq, vd, _ = ssm.answers(sc, key="tile")
    assert np.array_equal(q, vq) and not np.array_equal(d.view(np.uint32), vd.view(np.uint32))


def test_first_occurrences_keep_the_order():
    t = np.array([(3, 4), (3, 5), (3, 4), (2, 9), (3, 5), (0, 0)], np.int16)
    assert ssm.first_occurrences(t) == [(3, 4), (3, 5), (2, 9), (0, 0)]
