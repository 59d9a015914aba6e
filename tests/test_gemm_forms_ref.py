"""The references of tests/test_gemm_forms_gpu.py, checked without a GPU.

  * the numpy gather that stands for GemmArgs' implicit-conv addressing (cv_*, seg_len, seg_stride) against
    torch.nn.functional.conv2d in float64 on the same NHWC input: the mapping is the part of that file most easily written wrong;
  * every case of tests/gemm_forms.py with a float32 numpy product (and float32 epilogue) in the kernel's place: the float64
    reference and the stand-in must agree within the derived per-element tolerance, and that tolerance must stay under check()'s
    2e-5 ceiling -- a bound or a reference that is wrong fails here, before any kernel is involved.  The plan of every launch comes
    from csrc/gemm_plan.cpp itself (the sanitizer driver's `plans` command), so the plans each case is written to reach are
    asserted here as well."""
import os
import subprocess

import numpy as np
import pytest

import gemm_forms as gf
from test_kernels_gpu import check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API_DRIVER = os.path.join(ROOT, "tests", "native", "k2hip_san_api_driver")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san"])
    path = str(tmp_path_factory.mktemp("plans") / "line.txt")

    def ask(line):
        with open(path, "w") as f:
            f.write(line + "\n")
        r = subprocess.run([API_DRIVER, "plans", path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (line, r.stderr[-2000:])
        return r.stdout.strip().split(" -> ")[1].split()
    return ask


@pytest.mark.parametrize("C,st,sf,N", [(8, 2, 2, 32), (32, 1, 2, 128), (32, 2, 2, 128)])
def test_conv_gather_reference_is_conv2d(C, st, sf, N):
    """row r = (b Tout + t) Fout + f reads x[b, t st + kt, f sf + kf, c] at k = (kt 3 + kf) C + c: a 3 x 3 convolution, stride
    (st, sf), no padding, weight[o, c, kt, kf] = W[o, (kt 3 + kf) C + c], output [B, Tout, Fout, N] row-major"""
    import torch
    rng = np.random.default_rng(C + st)
    B, Tin, Fin = 2, 11, 15
    g = gf.conv_launch(rng, f"conv2d C={C} st={st}", B, Tin, Fin, C, st, sf, N, act=gf.ACT_NONE)
    want, _, written = g.reference()
    assert written.sum() == g.f["M"] * N
    x = torch.from_numpy(g.A[:B * Tin * Fin * C].astype(np.float64).reshape(B, Tin, Fin, C)).permute(0, 3, 1, 2)
    w = torch.from_numpy(g.W[:N * 9 * C].astype(np.float64).reshape(N, 3, 3, C)).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(x, w, torch.from_numpy(g.bias.astype(np.float64)), stride=(st, sf))
    assert tuple(y.shape) == (B, N, g.f["cv_Tout"], g.f["cv_Fout"])
    y = y.permute(0, 2, 3, 1).reshape(-1, N).numpy()
    assert np.abs(want[written].reshape(-1, N) - y).max() <= 1e-13


@pytest.mark.parametrize("k", range(len(gf.CASES)))
def test_float32_standin_passes_every_case(plans, k):
    case = gf.CASES[k]

    def runner(launch):
        out = plans(launch.plan_line())
        assert out[0] != "error", (launch.what, "the plan refuses this launch")
        return gf.standin(launch), (out[0], int(out[1]))
    n, _ = gf.run_case(case, k + 1, runner, check)
    assert n >= case.floor


def test_float32_standin_passes_the_fused_conv_cases(plans):
    from test_gemm_forms_gpu import glu_conv_operands, glu_conv_reference
    rng = np.random.default_rng(10)
    for B, Tc, D, K, want_entry in gf.CONV_SHAPES:
        assert plans(f"conv {B} {Tc} {D} {K}") == ["ring", str(want_entry)]
        ops = glu_conv_operands(rng, B, Tc, D, K)
        want, tol, cache, ctol = glu_conv_reference(*ops, B, Tc, D, K)
        got, _, got_cache, _ = glu_conv_reference(*ops, B, Tc, D, K, dt=np.float32)
        check(got, want, tol, f"stand-in B={B} Tc={Tc} D={D} K={K}")
        check(got_cache, cache, ctol, f"stand-in cache B={B} Tc={Tc} D={D} K={K}")
    for B, Tc, D, K in gf.CONV_REFUSED:
        assert plans(f"conv {B} {Tc} {D} {K}") == ["none"]
