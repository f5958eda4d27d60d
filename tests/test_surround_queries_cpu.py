"""The numpy model of the surround queries (tests/surround_model.py) is pinned to the reference build: on every world of
the GPU file it gives RefMove.surround_queries' bytes and floats (compared as uint32), and each of eight plausible
mistakes -- the `variant`s of the model -- changes at least one answer on those worlds, so the worlds can tell them apart.
No GPU; skipped where oracle/_ref is absent."""
import numpy as np
import pytest

from oracle import pfref
from tests import surround_model as sm

pytestmark = pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")

VARIANTS = ["le", "colmajor", "centres", "start_unvisited", "four", "ignore_blockers", "dest_island", "vel_both"]


@pytest.mark.parametrize("name", sorted(sm.WORLDS))
def test_model_equals_the_reference(name):
    w = sm.world(name)
    q, d, info = w.answers()
    nav = sm.ref_nav(w)
    try:
        for l in w.blockers:
            assert np.array_equal(sm.to_chunks(w.islands), nav.plane(pfref.PLANE_ISLANDS, l))
        rq, rd = sm.ref_answers(w, nav)
    finally:
        nav.close()
    host = q == sm.SQ_HOST                   # (the rows the device leaves to the host: the reference answers them)
    assert host.sum() == (2 if name == "beyond_the_window" else 0)
    assert np.array_equal(q[~host], rq[~host]) and np.array_equal(d[~host].view(np.uint32), rd[~host].view(np.uint32))
    assert (rq[host] != 0).all()
    assert (w.target >= 0).sum() == sum(1 for inf in info if inf) > 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_wrong_model_changes_an_answer(variant):
    changed = []
    for name in sorted(sm.WORLDS):
        w = sm.world(name)
        q, d, _ = w.answers()
        vq, vd, _ = w.answers(variant)
        if not (np.array_equal(q, vq) and np.array_equal(d.view(np.uint32), vd.view(np.uint32))):
            changed.append(name)
    assert changed, variant


def test_the_benchmark_like_batch_repeats_floods():
    """Many units surround one target from one island: the share of floods that repeat another row's (target, layer,
    island) in a small batch of the benchmark's kind (DESIGN.md 11 quotes the share of the measured batches)."""
    w = sm.bench_like(64, 8, w=2, h=2)
    share = w.duplicate_flood_share()
    assert 0.5 < share < 1.0, share
