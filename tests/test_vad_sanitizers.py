"""The host side of the voice activity detector as its own program under AddressSanitizer / UBSan (tests/native/san_vad_driver.cpp,
`make san_vad`): the float32 reference over random configs and chunkings, the carried-state bookkeeping of the streams -- features and
samples in any chunking, remainders, another sample rate, the rate rules --, create / reset / flush / pop / destroy in every order, and
the long entry's packing and result object, all through the C ABI over the CPU stand-ins of the engine."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_side_under_the_sanitizers(tiny_model_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_vad"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_vad_driver"), tiny_model_path], capture_output=True, text=True, env=env,
                       timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_vad_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
