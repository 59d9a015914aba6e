"""The host side of the neural LM shallow fusion as its own program under AddressSanitizer / UBSan
(tests/native/san_rnn_lm_fusion_driver.cpp, `make san_rnn_lm_fusion`): the fused search's weight layout (csrc/rnn_lm_fuse_layout.h) on
LMs of every shape class -- E == H, E below a multiple of 32 (padded input columns), E != H with three layers -- element by element
against its definition, and the switch with the LM set, replaced and cleared in every order through the C ABI over the CPU stand-ins of
the engine.  Nothing is preloaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_side_under_the_sanitizers(tiny_model_path, tmp_path):
    from k2transducerasr_amd.synth import write_synthetic_rnn_lm
    lms = []
    for i, (E, H, L) in enumerate([(64, 64, 1), (20, 32, 2), (32, 96, 3)]):
        p = str(tmp_path / f"lm{i}.k2w")
        write_synthetic_rnn_lm(p, 37, E, H, L, 20 + i)
        lms.append(p)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_rnn_lm_fusion"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_rnn_lm_fusion_driver"), tiny_model_path] + lms, capture_output=True, text=True,
                       env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_rnn_lm_fusion_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
