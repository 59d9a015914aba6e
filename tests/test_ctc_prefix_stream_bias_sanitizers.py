"""The host side of biasing in the streaming CTC prefix beam search as its own program under AddressSanitizer / UBSan
(tests/native/san_ctc_prefix_stream_bias_driver.cpp, `make san_ctc_prefix_stream_bias`): random rows with random graphs and LMs at
random chunkings through csrc/ctc_prefix_hist.h with its side blocks and the float32 reference of the resumed biased step, after every
chunk bit for bit csrc/ctc_prefix_bias_ref.h over the frames so far; side blocks with states out of range; and the per-stream setters,
shared graphs, destroy orders and the LM-change rule through the C ABI over the CPU stand-ins of the engine."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_side_under_the_sanitizers(tiny_model_path, tmp_path):
    from k2transducerasr_amd.synth import write_synthetic_model
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_ctc_prefix_stream_bias"])
    ctc = str(tmp_path / "ctc.k2w")
    write_synthetic_model(ctc, "zipformer2-ctc-tiny-test")
    ctc_streaming = str(tmp_path / "ctc_streaming.k2w")
    write_synthetic_model(ctc_streaming, "zipformer2-ctc-streaming-tiny-test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_ctc_prefix_stream_bias_driver"), ctc, tiny_model_path, ctc_streaming],
                       capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_ctc_prefix_stream_bias_driver ok (180 cases" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
