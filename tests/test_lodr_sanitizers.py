"""The host side of LODR as its own program under AddressSanitizer / UBSan (tests/native/san_lodr_driver.cpp, `make san_lodr`):
BeamHistory with the LODR plane across begin / fill / apply / reset and the setting-change rule of the streaming entries, and the host
rescoring walk (csrc/lodr_host.h) over random automata against the unscaled step.  Nothing is preloaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_side_under_the_sanitizers():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_lodr"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_lodr_driver")], capture_output=True, text=True, env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_lodr_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
