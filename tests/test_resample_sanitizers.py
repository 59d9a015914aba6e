"""The host side of the sample-rate converter as its own program under AddressSanitizer / UBSan (tests/native/san_resample_driver.cpp,
`make san_resample`): the plan builder and the float32 reference over random rates and chunkings, and the streams' bookkeeping at
other sample rates -- counts, the queue erase, the rate rules, reset -- through the C ABI over the CPU stand-ins of the engine."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_side_under_the_sanitizers(tiny_model_path, tmp_path):
    from k2transducerasr_amd.synth import write_synthetic_model
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_resample"])
    streaming = str(tmp_path / "stiny.k2w")
    write_synthetic_model(streaming, "zipformer2-streaming-tiny-test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_resample_driver"), tiny_model_path, streaming], capture_output=True,
                       text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_resample_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
