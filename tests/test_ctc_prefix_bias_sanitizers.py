"""The host side of the biased CTC prefix beam search as its own program under AddressSanitizer / UBSan
(tests/native/san_ctc_prefix_bias_driver.cpp, `make san_ctc_prefix_bias`): csrc/ctc_prefix_bias_ref.h against brute force, against
ctc_prefix_ref.h with null and with empty tables bit for bit, random graphs and LMs, the table check on broken tables, and
k2hip_set_ctc_prefix_biasing with the operator entry around it through the C ABI over the CPU stand-ins of the engine."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_side_under_the_sanitizers(tiny_model_path, tmp_path):
    from k2transducerasr_amd.synth import write_synthetic_model
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_ctc_prefix_bias"])
    ctc = str(tmp_path / "ctc.k2w")
    write_synthetic_model(ctc, "zipformer2-ctc-tiny-test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_ctc_prefix_bias_driver"), ctc, tiny_model_path], capture_output=True,
                       text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_ctc_prefix_bias_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
