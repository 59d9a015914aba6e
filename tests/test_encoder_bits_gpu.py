"""The Zipformer2 and Zipformer v1 encoders, offline and streaming, bit for bit against tests/golden/encoder_bits_golden.json: SHA-1
digests of outputs, taps and streaming caches, the token lists, and the integer columns of the GEMM launch log, as recorded on an
MI355X by tools/make_encoder_bits_golden.py (the cases are its functions; the encoder has no floating-point atomics).  A change to
the host orchestration must leave every entry as it is; each test asserts the weights' checksum first, so that another synthetic
model reads as "different weights" and not as a broken encoder."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    import make_encoder_bits_golden as rec
    with open(rec.GOLDEN) as fh:
        return json.load(fh)


def _leaves(tree, at=""):
    """every entry of a recorded case by its path ("default.tap3", "state.0.4.key"); a launch log is one entry per row"""
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _leaves(tree[k], f"{at}.{k}" if at else k)
    elif isinstance(tree, list) and tree and isinstance(tree[0], (dict, list)):
        for i, v in enumerate(tree):
            yield from _leaves(v, f"{at}.{i}")
    else:
        yield at, tree


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f"])
def test_encoder_bits(golden, tmp_path_factory, case):
    import make_encoder_bits_golden as rec
    got = rec.run_case(case, str(tmp_path_factory.getbasetemp()))
    want = golden[case]
    assert got["weights"] == want["weights"], "the synthetic model's weights are not the ones the fixture was recorded with"
    got, want = dict(_leaves(got["got"])), dict(_leaves(want["got"]))
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, f"{len(differ)} of {len(want)} entries differ from the fixture, first: {differ[0]}: {got[differ[0]]} != {want[differ[0]]}"
