"""The image-side convolution family (the Bottleneck convolution forward, data and weight gradients; the necks' lateral forward,
data and weight gradients; rac_conv3x3_wgrad; rac_linear_wgrad) returns a pin of the parent build bit for bit
(tests/golden/gen_conv_family_pin.py): every kernel instance and every branch of the code these kernels share."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu


def test_conv_family_matches_the_parent_build(golden_dir):
    from golden import gen_conv_family_pin as pin
    with open(os.path.join(golden_dir, "conv_family_pin.json")) as f:
        want = json.load(f)
    d = pin.inputs()
    assert {k: pin.digest(v) for k, v in d.items()} == want["inputs"], "the seeded inputs are not those of the pin"
    got = pin.outputs(d)
    assert sorted(got) == sorted(want["outputs"]) and len(got) == 47
    wrong = [name for name, v in got.items() if pin.digest(v) != want["outputs"][name]]
    assert not wrong, wrong
