"""The fixture tests/golden/decoder_grad_small.npz pinned without a GPU: the reference's own float32 gradients stored in it, and
the package's torch comparator route -- the layer's forward_train with the HIP launchers replaced by the float64 torch fakes of the
module tests (tests/test_decoder_grad_cpu.py's ``fakes``: float64 inside, float32 at their boundary), float32 torch layers around them -- both against the stored float64 gradients of
the reference, per tensor, within max(2 x the reference's own float32 figure, 1e-5) of the tensor's largest element."""
import numpy as np
import pytest
import torch

import decoder_grad_ref as DR
from test_decoder_grad_cpu import fakes  # noqa: F401  (fixture)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return DR.load_golden(golden_dir)


def test_fixture_is_consistent(golden):
    g = golden
    names = sorted(k[4:] for k in g if k.startswith("g64:"))
    assert len(names) == 104 and {"query_bbox", "query_feat", "lss", "radar", "feat0", "feat3"} <= set(names)
    for k in names:
        assert g["g32:" + k].dtype == np.float32 and g["g64:" + k].dtype == np.float64 and g["g32:" + k].shape == g["g64:" + k].shape
        assert float(g["max64:" + k]) > 0
        # the stored figure covers the whole tensor, so it bounds the kept entries
        assert DR.rel_err(g["g32:" + k], g["g64:" + k], float(g["max64:" + k])) <= float(g["ref:" + k])
    assert np.abs(g["g64:query_bbox"].reshape(-1, 10)[:, 8:]).max() == 0, "the reference detaches the velocity"
    d = DR.draw(int(g["seed"]))
    assert all(np.array_equal(d[k], np.asarray(g[k]).astype(np.float32)) for k in d), "the inputs are the seed's"


def test_comparator_route_matches_the_reference(golden, fakes):  # noqa: F811
    layer = DR.build_layer(golden)
    out, grads = DR.run_layer(layer, golden)
    report = []
    bad = DR.check_against_golden(golden, out, grads, "comparator", report)
    worst = sorted(report, key=lambda r: -r[1] / r[3])[:5]
    print("\nclosest to the bound:", ", ".join(f"{k} {e:.1e} (ref {r:.1e})" for k, e, r, _ in worst))
    assert not bad, "\n".join(bad)
