"""The kernels around the encoder layers -- the offline front end, the streaming state movers, the small float4 kernels and the search
tail -- one launch at a time against float64, as tests/test_kernels_gpu.py and tests/test_family_kernels_gpu.py do for the layers'
own kernels: operands between NaN guards, pure outputs pre-filled with NaN, state pools and FIFOs compared bit for bit including
every float a launch must not touch, integer results exact.  The cases, the float64 references and the derivation of every
tolerance are in tests/outer_kernels.py; tests/test_outer_kernels_ref.py runs the same cases without a GPU and shows that each of
them rejects a deliberately wrong stand-in.  The whole-model tests hold these kernels only through token parity and feature
comparisons at 2e-5 to 5e-4 on inputs that avoid their edges."""
import pytest

import outer_kernels as ok
from test_kernels_gpu import op, switch  # noqa: F401  (op: the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", range(len(ok.CASES)), ids=[name.replace(" ", "_") for name, _ in ok.CASES])
def test_outer_kernel(op, k):
    ok.RATIO[0] = 0.0
    ok.CASES[k][1](ok.Env(op, switch))
    print(f"{ok.CASES[k][0]}: largest error / tolerance {ok.RATIO[0]:.3f}")
