"""The kernels of the Conformer, Zipformer v1 and LSTM families (csrc/conformer.hip, zipformer1.hip, lstm.hip, and basicnorm / conv0 of
elementwise.hip) one launch at a time against float64, as tests/test_kernels_gpu.py does for the Zipformer2 kernels: operands
between NaN guards, outputs pre-filled with NaN, pad columns exactly 0.0, row strides wider than the rows, state-pool floats a
launch must not touch compared bit for bit.  The cases, the float64 references and the derivation of every tolerance are in
tests/family_kernels.py (tests/test_family_kernels_ref.py runs the same cases without a GPU and holds the references to the torch
twins); the whole-model tests (test_conformer_gpu.py, test_zipformer1_gpu.py, test_lstm_gpu.py) hold these kernels to the float32
oracle at 2e-4 and wider, where one slightly wrong branch can hide."""
import pytest

import family_kernels as fk
from test_kernels_gpu import op, switch  # noqa: F401  (op: the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", range(len(fk.CASES)), ids=[name.replace(" ", "_") for name, _ in fk.CASES])
def test_family_kernel(op, k):
    fk.CASES[k][1](fk.Env(op, switch))

