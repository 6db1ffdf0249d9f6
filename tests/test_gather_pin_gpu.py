"""The gather forwards (rac_msmv_fwd, rac_msmv_v2_fwd, rac_msda_fwd) and the single-writer gradients of rac_msda_bwd return
a pin of the parent build bit for bit (tests/golden/gen_gather_fwd_pin.py): every kernel instance, finite locations only,
out-of-range ones included."""
import json
import os

import pytest

from racformer_amd import _lib

pytestmark = pytest.mark.gpu


def test_gathers_match_the_parent_build(golden_dir):
    from golden import gen_gather_fwd_pin as pin
    with open(os.path.join(golden_dir, "gather_fwd_pin.json")) as f:
        want = json.load(f)
    d = pin.inputs()
    assert {k: pin.digest(v) for k, v in d.items()} == want["inputs"], "the seeded inputs are not those of the pin"
    got = pin.outputs(_lib.lib(), d)
    assert sorted(got) == sorted(want["outputs"]) and len(got) == 38
    for name, v in got.items():
        assert pin.digest(v) == want["outputs"][name], name
